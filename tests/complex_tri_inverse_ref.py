"""Reference, inputs and residual measure of the complex triangular-inverse tests (test_complex_tri_inverse_abi.py and
test_ctrtri_host.py on the CPU, test_gpu_complex_tri_inverse.py on the device).  Nothing here needs a GPU.

Yardstick: recursive_inverse() restates the reference's recursion (faer/src/linalg/triangular_inverse.rs:43-123) in numpy, in the
working precision, by halves down to 1 x 1: invert the two diagonal halves, W10 = -T10 W00, then solve T11 X = W10 by substitution.

Measure: residual(T, W) = max over both sides of  max_ij |T W - I|_ij / (|T| |W|)_ij  evaluated in clongdouble on the triangle the call
works on (entries whose denominator is zero have a zero numerator too and count as 0).  A case passes when
    residual(T, W_gpu) <= FACTOR * max(residual(T, W_ref), eps):
the floor eps is one rounding of an entry -- for n = 1 the reference's quotient can be exact (residual 0) where a correctly rounded
reciprocal of another form is not."""
import functools

import numpy as np

from complex_cases import ext, ceps, tri_matrix, tri_poisoned, substitute, gauss_int  # noqa: F401  (re-exported for the tests)

VARIANTS = (("lower", False), ("upper", False), ("lower", True), ("upper", True))  # (triangle, unit)
# Admitted factor over the yardstick: twice the largest r_gpu / max(r_ref, eps) recorded in profiles/complex_tri_inverse_error.txt on
# one MI355X, rounded up to an integer, never below 2.  A ratio above 16 is a defect of the kernel, not a tolerance to widen.
FACTOR = 5
NAN_SENTINEL = {np.dtype(np.complex64): np.uint32(0x7FC0BEEF), np.dtype(np.complex128): np.uint64(0x7FF80000DEADBEEF)}


def sizes(e, sub_blocks):
    """the sizes at which the kernel can go wrong, for a leaf of edge e with `sub_blocks` sub-blocks along it"""
    sb = e // sub_blocks
    out = {1, 2, e - 1, e, e + 1, 2 * e, 2 * e + 1, 3 * e + 5, 4 * e + e // 2}
    for k in range(1, sub_blocks):
        out |= {k * sb - 1, k * sb + 1}
    return sorted(out)


def effective(t, triangle, unit):
    """the matrix the operand stands for: its triangle, zeros outside, ones on a unit diagonal"""
    out = (np.tril(t) if triangle == "lower" else np.triu(t)).copy()
    if unit:
        np.fill_diagonal(out, 1)
    return out


def _lower(t, unit):
    n = t.shape[0]
    if n == 0:
        return t.copy()
    if n == 1:
        return np.ones_like(t) if unit else (t.dtype.type(1) / t).astype(t.dtype)
    h = n // 2
    w = np.zeros_like(t)
    w[:h, :h] = _lower(t[:h, :h], unit)
    w[h:, h:] = _lower(t[h:, h:], unit)
    bl = (-(t[h:, :h] @ w[:h, :h])).astype(t.dtype)
    w[h:, :h] = substitute(np.ascontiguousarray(t[h:, h:]), bl, "lower", unit, False)
    return w


def recursive_inverse(t, triangle, unit):
    """the inverse of the (unit) triangle of t, as a full matrix in t's precision"""
    te = effective(t, triangle, unit)
    if triangle == "upper":
        return np.ascontiguousarray(_lower(np.ascontiguousarray(te.T), unit).T)
    return _lower(te, unit)


def residual(t, w, triangle, unit):
    """w: the full inverse (its triangle; a unit diagonal is taken as one whatever w holds)"""
    we = effective(w, triangle, unit)
    if not np.isfinite(we).all():
        return np.inf
    te, we = ext(effective(t, triangle, unit)), ext(we)
    eye = np.eye(t.shape[0], dtype=np.clongdouble)
    worst = 0.0
    for a, b in ((te, we), (we, te)):
        num, den = np.abs(a @ b - eye), np.abs(a) @ np.abs(b)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(num == 0, 0, num / den)
        worst = max(worst, float(q.max()) if q.size else 0.0)
    return worst


@functools.lru_cache(maxsize=None)
def case(n, dtype, triangle, unit):
    """(T clean, T poisoned, W_ref, r_ref): tri_matrix of the ctrsm tests; computed once, never written"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(n * 7919 + (3 if triangle == "upper" else 0) + (5 if unit else 0) + (11 if dt == np.complex64 else 0))
    t = tri_matrix(rng, n, dt, triangle, unit)
    tp = tri_poisoned(t, triangle, unit)
    w = recursive_inverse(t, triangle, unit)
    r = residual(t, w, triangle, unit)
    for x in (t, tp, w):
        x.setflags(write=False)
    return t, tp, w, r


def yardstick(r_ref, dtype):
    return max(r_ref, ceps(dtype))


def sentinel(n, dtype):
    """n x n, column major, every real and imaginary part a NaN with a payload: a destination nothing has written yet"""
    dt = np.dtype(dtype)
    bits = NAN_SENTINEL[dt]
    return np.asfortranarray(np.full((n, n, 2), bits, dtype=bits.dtype).view(dt)[:, :, 0])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def written_mask(n, triangle, unit):
    i, j = np.indices((n, n))
    m = (i >= j) if triangle == "lower" else (i <= j)
    return m & (i != j) if unit else m


UNITS = np.array([1, -1, 1j, -1j])
DIAGS = np.array([1, -1, 1j, -1j, 2, -2, 0.5, -0.5, 2j, -2j])


def exact_case(n, dtype, triangle, unit, seed=0):
    """(T, W): T is the identity plus a first sub-diagonal drawn from {+-1, +-i} (non-unit: a diagonal drawn from {+-1, +-i, +-2,
    +-1/2, +-2i}); W(i, j) = (-1)^(i-j) prod_{j<=k<i} t(k+1, k) / prod_{j<=k<=i} d(k), a unit times a power of two, built here from
    exact cumulative products in complex128 (the exponents stay within +-60 for the sizes used: asserted).  Every sum of an inversion
    by substitution or by block products has at most one non-zero term, so any correct schedule reproduces W exactly."""
    rng = np.random.default_rng(1000 * n + seed + (1 if unit else 0))
    sub = UNITS[rng.integers(0, 4, max(n - 1, 0))]
    d = np.ones(n, dtype=np.complex128) if unit else DIAGS[rng.integers(0, len(DIAGS), n)]
    t = np.diag(d) + np.diag(sub, -1)
    w = np.zeros((n, n), dtype=np.complex128)
    for j in range(n):
        w[j, j] = 1 / d[j]
        for i in range(j + 1, n):
            w[i, j] = -w[i - 1, j] * sub[i - 1] / d[i]
    mag = np.abs(w[np.tril_indices(n)])
    assert mag.min() >= 2.0 ** -60 and mag.max() <= 2.0 ** 60
    if triangle == "upper":
        t, w = t.T, w.T
    tt, ww = np.asarray(t, dtype=dtype, order="F"), np.asarray(w, dtype=dtype, order="F")
    assert np.array_equal(ww.astype(np.complex128), w)
    return tt, ww
