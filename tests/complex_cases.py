"""Inputs, references and bounds of the complex level-3 tests (test_complex_abi.py on the CPU, test_gpu_complex_matmul.py and
test_gpu_complex_trsm.py on the device).  References are numpy in clongdouble; nothing here needs a GPU.

Bounds (componentwise, moduli):
  product  |got - ref| <= 4 (K + 2) eps (|alpha| (|A||B|) + |C0|): the project's 4 K eps widened by the sqrt(2) gamma_2 of a
           conventional complex product, one complex scaling by alpha and one addition (Higham, Accuracy and Stability, section 3.6);
           sqrt(2) (K + 4) + 1 <= 4 (K + 2) for every K >= 0.
  solve    |op(T) X - B| <= 12 n eps (|T||X| + |B|): the project's C_TRI = 4 times the 2 sqrt(2) by which a complex multiply or divide
           exceeds a real one."""
import functools

import numpy as np

CDTYPES = (np.complex64, np.complex128)
MATMUL_SHAPES = [(1, 1, 1), (15, 16, 17), (17, 15, 16), (127, 129, 128), (129, 127, 130), (5, 7, 0), (64, 1, 33), (1, 70, 9),
                 (130, 130, 70), (300, 200, 1000)]
MATMUL_MODES = (("add", -0.5 + 0.25j), ("replace", 2 - 1j))
TRSM_SIZES = (1, 2, 63, 64, 65, 129, 300)
TRSM_NRHS = (1, 33)
TRSM_VARIANTS = (("lower", False), ("upper", False), ("lower", True), ("upper", True))  # (triangle, unit)
C_TRI_COMPLEX = 12
BLOCKS = ("rect", "lower", "upper", "strict_lower", "strict_upper", "unit_lower", "unit_upper")


def ceps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)  # (of the real type underneath)


def crandn(rng, m, n, dtype):
    return np.asarray(rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n)), dtype=dtype, order="F")


def gauss_int(rng, m, n, dtype, lim=3):
    return np.asarray(rng.integers(-lim, lim + 1, (m, n)) + 1j * rng.integers(-lim, lim + 1, (m, n)), dtype=dtype, order="F")


def ext(x):
    return np.asarray(x, dtype=np.clongdouble)


# ---- product
@functools.lru_cache(maxsize=None)
def matmul_case(m, n, k, dtype):
    """(a, b, c0, A B in clongdouble, |A||B| in longdouble); computed once, never written"""
    rng = np.random.default_rng(m * 1000003 + n * 1009 + k + (7 if np.dtype(dtype) == np.complex64 else 0))
    a, b, c0 = crandn(rng, m, k, dtype), crandn(rng, k, n, dtype), crandn(rng, m, n, dtype)
    prod = ext(a) @ ext(b)
    mag = np.abs(ext(a)) @ np.abs(ext(b))
    for x in (a, b, c0, prod, mag):
        x.setflags(write=False)
    return a, b, c0, prod, mag


def matmul_ref_and_bound(m, n, k, dtype, mode, alpha):
    a, b, c0, prod, mag = matmul_case(m, n, k, dtype)
    al = np.clongdouble(alpha)
    ref = al * prod + (ext(c0) if mode == "add" else 0)
    bound = 4 * (k + 2) * ceps(dtype) * (abs(al) * mag + (np.abs(ext(c0)) if mode == "add" else 0))
    return ref, bound


# ---- FaerBlock structure (faer/src/linalg/matmul/triangular.rs:906-977)
def block_mask(kind, n_rows, n_cols):
    i, j = np.indices((n_rows, n_cols))
    return {"rect": np.ones((n_rows, n_cols), bool), "lower": i >= j, "upper": i <= j, "strict_lower": i > j, "strict_upper": i < j,
            "unit_lower": i > j, "unit_upper": i < j}[kind]


def block_effective(x, kind):
    """the matrix a structured operand stands for: zero outside the block, ones on an implicit unit diagonal"""
    out = np.where(block_mask(kind, *x.shape), x, 0).astype(x.dtype)
    if kind.startswith("unit"):
        np.fill_diagonal(out, 1)
    return out


def block_poisoned(x, kind):
    """the operand as it is handed over: NaN wherever the block kind says the entry is not accessed"""
    return np.asfortranarray(np.where(block_mask(kind, *x.shape), x, np.nan + 1j * np.nan).astype(x.dtype))


# ---- triangular solves
def tri_matrix(rng, n, dtype, triangle, unit):
    """tril(randn + i randn) / n + I, or its transpose or unit form; the other triangle (and a unit diagonal) is NaN: never read"""
    t = np.tril(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / n + np.eye(n)
    if unit:
        np.fill_diagonal(t, 1)
    if triangle == "upper":
        t = t.T
    return np.asarray(t, dtype=dtype, order="F")


def tri_poisoned(t, triangle, unit):
    i, j = np.indices(t.shape)
    read = (i >= j) if triangle == "lower" else (i <= j)
    if unit:
        read &= i != j
    return np.asfortranarray(np.where(read, t, np.nan + 1j * np.nan).astype(t.dtype))


@functools.lru_cache(maxsize=None)
def trsm_case(n, nrhs, dtype, triangle, unit):
    rng = np.random.default_rng(n * 7919 + nrhs * 31 + (3 if triangle == "upper" else 0) + (5 if unit else 0))
    t, b = tri_matrix(rng, n, dtype, triangle, unit), crandn(rng, n, nrhs, dtype)
    t.setflags(write=False)
    b.setflags(write=False)
    return t, b


def tri_backward_error(t, x, b, conj, c=C_TRI_COMPLEX):
    """max over the entries of |op(T) X - B| / (c n eps (|T||X| + |B|)) in clongdouble (<= 1 passes); non-finite X: inf.
    (stability_cases.tri_backward_error casts to longdouble and would drop the imaginary parts.)"""
    if not np.isfinite(x).all():
        return np.inf
    n = t.shape[0]
    te, xe, be = ext(np.conj(t) if conj else t), ext(x), ext(b)
    res = np.abs(te @ xe - be)
    scale = c * max(n, 1) * ceps(t.dtype) * (np.abs(te) @ np.abs(xe) + np.abs(be))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(res == 0, 0, res / scale)
    return float(q.max()) if q.size else 0.0


def substitute(t, b, triangle, unit, conj):
    """plain substitution in the working precision: the yardstick's own reachability check"""
    n = t.shape[0]
    tt = np.conj(t) if conj else t
    x = b.copy()
    order = range(n) if triangle == "lower" else range(n - 1, -1, -1)
    for i in order:
        js = slice(0, i) if triangle == "lower" else slice(i + 1, n)
        acc = x[i] - tt[i, js] @ x[js]
        x[i] = acc if unit else acc / tt[i, i]
    return x


UNIT_ENTRIES = np.array([0, 1, -1, 1j, -1j])
DIAG_ENTRIES = np.array([1, -1, 1j, -1j, 2, -2, 2j, -2j, 0.5, -0.5])


def exact_trsm_case(n, nrhs, dtype, triangle, unit, conj, seed=0):
    """(T, B, X0): strictly triangular entries in {0, +-1, +-i}, a non-unit diagonal from {+-1, +-i, +-2, +-2i, +-1/2}, X0 Gaussian
    integers, B = op(T) X0 -- every intermediate of a substitution is a Gaussian half-integer far below 2^24: the solve is exact"""
    rng = np.random.default_rng(n * 131 + nrhs + seed)
    t = np.tril(UNIT_ENTRIES[rng.integers(0, len(UNIT_ENTRIES), (n, n))], -1)
    t = t + np.diag(np.ones(n) if unit else DIAG_ENTRIES[rng.integers(0, len(DIAG_ENTRIES), n)])
    if triangle == "upper":
        t = t.T
    x0 = gauss_int(rng, n, nrhs, np.complex128)
    b = (np.conj(t) if conj else t) @ x0
    return np.asarray(t, dtype=dtype, order="F"), np.asarray(b, dtype=dtype, order="F"), np.asarray(x0, dtype=dtype, order="F")
