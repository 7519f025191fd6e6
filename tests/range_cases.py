"""Inputs at the ends of the floating-point range (CPU only): the scale tables, the generators and the comparisons shared by
tests/test_range_cases.py (the references alone, no GPU) and tests/test_gpu_range_edges.py (the kernels against them).

Every scale is an exact power of two, 2.0 ** k, so scaling commits no rounding: a factorization without an absolute threshold
returns the same reflectors, taus, T factors and permutations for A and 2^k A, and 2^k times the parts that carry the scale.
A family is described by
  * its cases (shapes) and the generator of the unscaled input,
  * IN_EXP: the input is A * 2^(IN_EXP k) (2 for the Cholesky-type families, whose factor then carries 2^k),
  * its reference, returning {part: (array, e)}: the part scales with 2^(e k),
  * its comparison, which works on UNSCALED parts (every part times 2^(-e k), exact) with the bound of the family's existing
    oracle test unchanged: dividing by the scale is the same as multiplying that test's ||A|| by it.

K[family][dtype] = (-extreme, -moderate, +moderate, +extreme).  The moderate scales stay inside every fast path (the v_rsq_f64
chain of potrf.hip, the one-pass QR guard, plain sums of squares); the extreme ones cross 2^+-511 (fp64) / 2^+-63 (fp32), where the
three-accumulator norm switches accumulator, and for Cholesky put the pivots beyond 1e+-280.  The values below are the largest
that cap_ok accepts for every case of the family, input and reference output (tests/test_range_cases.py asserts it):
  * fp64, 2^+-900: the format ends at 2^+-1022; a Gaussian entry of relative size 2^-20 and a norm of 2^10 leave ~100 binades
    of room on both sides.  (tests/test_gpu_qr.py already goes to 1e+-250 ~ 2^+-830.)
  * fp32, 2^+100 / 2^-90: norms up to 2^9 times 2^100 stay below 2^127; the small side is limited by the smallest entries of
    the outputs (2^-90 times an entry of relative size 2^-30 is still normal).
  * Cholesky (A * 4^k): fp64 k = +-480 (pivots ~ 1e+-289 n), fp32 k = +-50.
  * pivoted QR with individually scaled columns (GRADED_KX): the reference multiplies the whole matrix by 1 / (largest column
    norm) first (qr/col_pivoting/factor.rs:142-160), so the SPREAD of the column scales, not their position, is what the format
    limits: an entry of relative size 2^-20 of the smallest column, 2^(-2 kx - 24) after that scaling, must stay normal.
"""
import numpy as np

from gpu_util import EPS, boosted, quasi_definite, rnd, spd, sym, well_conditioned
from test_bidiag_oracle import bidiag_of
from test_hessenberg_oracle import hess_of
from test_tridiag_oracle import tridiag_of

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = [np.float64, np.float32]

GENERAL = {F64: (-900, -100, 100, 900), F32: (-90, -20, 20, 100)}
CHOLESKY = {F64: (-480, -50, 50, 480), F32: (-50, -10, 10, 50)}
GRADED_KX = {F64: 480, F32: 45}
K = {
    "tridiag": GENERAL, "bidiag": GENERAL, "hessenberg": GENERAL, "colpiv_qr": GENERAL, "qr": GENERAL,
    "lu": GENERAL, "fplu": GENERAL, "evd": GENERAL, "svd": GENERAL, "lblt": GENERAL,
    "llt": CHOLESKY, "ldlt": CHOLESKY, "piv_llt": CHOLESKY,
}
# the rank-deficient fp32 matrix of the general QR path: the dependent columns are rounding noise, eps times the scale, which must
# stay normal too: 2^-70, not 2^-90, on the small side
K["qr_deficient"] = {F64: GENERAL[F64], F32: (-70, -20, 20, 100)}
QR_DEFICIENT = (300, 120, 40)  # m, n, rank
IN_EXP = {f: (2 if f in ("llt", "ldlt", "piv_llt") else 1) for f in K}

# the shapes of the issue (condensed forms, pivoted QR: one per norm site of colpiv_qr.hip; plain QR: the four shapes of
# test_qr_norm_l2_scaling_cases, a blocked classic shape and one whose first panels have >= 1024 rows), the smallest sizes
# that reach the leaf and the blocked variant of each dense family (the lists of the dense tests)
CASES = {
    "tridiag": [5, 64, 333],
    "bidiag": [(7, 7), (300, 120), (120, 300)],
    "hessenberg": [6, 257],
    # (9, 10): wide, register body; (300, 120): several delayed updates; (40, 30, "C"): row major, every step recomputes the norms
    # (cp_step_kernel's helper blocks); (4100, 8): beyond 4096 rows, the memory-resident reflector body
    "colpiv_qr": [(9, 10, "F"), (300, 120, "F"), (40, 30, "C"), (4100, 8, "F")],
    "qr": [(9, 10), (1023, 5), (42, 1), (3000, 40), (300, 200), (1100, 400)],
    "llt": [100, 300],  # the leaf (n <= 128), the blocked recursion; the look-ahead driver: LLT_LOOKAHEAD_N
    "ldlt": [100, 300],
    "lu": [(33, 33), (300, 8), (257, 257), (8, 300)],
    "fplu": [(5, 5), (40, 30), (300, 300)],
    "lblt": [5, 64, 66, 130],
    "piv_llt": [5, 64, 66, 130],
}
LLT_LOOKAHEAD_N = 2048 + 2 * 128  # with FAER_HIP_LLT_LA_MIN=2048, FAER_HIP_LLT_TAIL=0 (tests/test_gpu_scratch_poison.py)


def pow2(k):
    return float(2.0 ** k)  # (exact in fp64 for |k| <= 1022; numpy casts it exactly to fp32 for |k| <= 126)


def cap_ok(x):
    """every entry finite and either exactly zero or a normal number of x's dtype"""
    x = np.asarray(x)
    assert x.dtype in (F64, F32)
    ax = np.abs(x)
    return bool(np.isfinite(x).all() and ((ax == 0) | (ax >= np.finfo(x.dtype).tiny)).all())


def cap_ok_taus(h):
    """cap_ok of a block of Householder factors, the +inf taus of empty tails excluded"""
    h = np.asarray(h)
    return cap_ok(np.where(np.isposinf(h), 0, h))


def scaled(a, k, e=1):
    """a * 2^(e k) in a's dtype, exactly (asserted through cap_ok by the callers)"""
    return np.asarray(a * a.dtype.type(pow2(e * k)), dtype=a.dtype, order="F" if a.flags.f_contiguous else "C")


def unscale(x, k, e):
    """x * 2^(-e k) in fp64 (exact: the result is O(1))"""
    return np.asarray(x, dtype=np.float64) * pow2(-e * k) if e else np.asarray(x, dtype=np.float64)


def unscaled_parts(parts, k):
    return {name: unscale(x, k, e) for name, (x, e) in parts.items()}


def make_input(family, case, dtype):
    """the unscaled input of a case: the generators of the existing tests, seeded by the case"""
    dtype = np.dtype(dtype).type
    if family in ("tridiag", "evd"):
        return sym(np.random.default_rng(case), case, dtype)
    if family in ("bidiag", "qr", "lu", "fplu", "svd"):
        m, n = case
        if family == "lu" and m == n:
            return well_conditioned(np.random.default_rng(m), m, dtype)
        return rnd(np.random.default_rng(m * 3 + n), m, n, dtype)
    if family == "hessenberg":
        return rnd(np.random.default_rng(case + 11), case, case, dtype)
    if family == "colpiv_qr":
        m, n, layout = case
        rng = np.random.default_rng(m * n)
        return np.array(rng.standard_normal((m, n)) * np.logspace(0, -3, n)[None, :], dtype=dtype, order=layout)
    if family == "llt":
        return spd(np.random.default_rng(case), case, dtype)
    if family == "ldlt":
        return quasi_definite(np.random.default_rng(case), case, dtype)[0]
    if family == "lblt":
        import lblt_ref

        return np.asarray(lblt_ref.random_symmetric(case, 1000 + case), dtype=dtype, order="F")
    if family == "piv_llt":
        return np.asarray(boosted(case), dtype=dtype, order="F")
    raise KeyError(family)


def rank_deficient(m, n, r, dtype):
    """product of an m x r and an r x n Gaussian matrix, rounded to dtype (tests/test_gpu_qr.py, the rank-deficient classic case)"""
    rng = np.random.default_rng(21)
    return np.asfortranarray((rnd(rng, m, r) @ rnd(rng, r, n)).astype(dtype))


def graded_columns(m, n, dtype, kx):
    """(a, g, c): a = g * c[None, :] with g Gaussian and the column scales c powers of two spread over 2^-kx .. 2^kx, shuffled;
    neighbouring scales differ by at least 2^2 and the norms of Gaussian columns of m >= 64 rows by less than 2, so no two column
    norms are within a factor of two and the pivot order has no ties"""
    rng = np.random.default_rng(m + n)
    g = rnd(rng, m, n, dtype)
    e = np.round(np.linspace(-kx, kx, n)).astype(int)
    assert n == 1 or np.diff(e).min() >= 2
    c = np.array([pow2(int(x)) for x in rng.permutation(e)])
    return np.asfortranarray(g * c[None, :].astype(dtype)), g, c


# ------------------------------------------------------------------------------------------------ references
def block_upper_mask(bs, size):
    tu = np.zeros((bs, size), bool)
    for j0 in range(0, size, bs):
        w = min(bs, size - j0)
        tu[:w, j0:j0 + w] = np.triu(np.ones((w, w), bool))
    return tu


def qr_block_size(O, m, n, dtype):
    return max(1, min(O.qr_recommended_block_size(m, n, dtype), min(m, n)))


def split_qr(qr, h):
    up = np.triu(np.ones(qr.shape, bool))
    return {"R": (np.where(up, qr, 0), 1), "V": (np.where(up, 0, qr), 0), "H": (h, 0)}


def reference(O, family, a, case=None):
    """({part: (array, e)}, exact): the reference's factors of `a` and what must agree exactly (permutations, counts, status)"""
    dt = a.dtype
    if family == "tridiag":
        n = a.shape[0]
        v, h = a.copy(order="F"), np.zeros((8, n - 1), dtype=dt, order="F")
        O.tridiag_in_place(v, h)
        return split_tridiag(v, h), {}
    if family == "bidiag":
        m, n = a.shape
        size = min(m, n)
        u, hl, hr = a.copy(order="F"), np.zeros((8, size), dtype=dt, order="F"), np.zeros((8, max(size - 1, 0)), dtype=dt, order="F")
        O.bidiag_in_place(u, hl, hr)
        return split_bidiag(u, hl, hr), {}
    if family == "hessenberg":
        n = a.shape[0]
        v, h = a.copy(order="F"), np.zeros((8, n - 1), dtype=dt, order="F")
        O.hessenberg_in_place(v, h)
        return split_hessenberg(v, h), {}
    if family == "colpiv_qr":
        m, n = a.shape
        bs = O.qr_recommended_block_size(m, n, dt)
        ref, h = a.copy(order="C" if a.flags.c_contiguous and not a.flags.f_contiguous else "F"), np.zeros((bs, min(m, n)), dtype=dt, order="F")
        cp, cpi, nt = O.colpiv_qr_in_place(ref, h)
        return split_qr(ref, h), {"perm": cp, "perm_inv": cpi, "count": nt}
    if family == "qr":
        m, n = a.shape
        bs = qr_block_size(O, m, n, dt)
        ref, h = a.copy(order="F"), np.zeros((bs, min(m, n)), dtype=dt, order="F")
        rank = O.qr_in_place(ref, h)
        return split_qr(ref, h), {"rank": rank}
    if family == "llt":  # numpy's Cholesky in fp64 of the input rounded to its dtype
        return {"L": (np.linalg.cholesky(a.astype(np.float64)), 1)}, {}
    if family == "ldlt":
        ref = a.copy(order="F")
        st = O.ldlt_in_place(ref)
        return {"L": (np.tril(ref, -1), 0), "D": (np.diag(ref).copy(), 2)}, {"status": st}
    if family == "lu":
        ref = a.copy(order="F")
        p, pi, nt = O.lu_in_place(ref)
        return {"L": (np.tril(ref, -1), 0), "U": (np.triu(ref), 1)}, {"perm": p, "perm_inv": pi, "count": nt}
    if family == "fplu":
        ref = a.copy(order="F")
        rp, rpi, cp, cpi, nt = O.full_piv_lu_in_place(ref)
        return {"L": (np.tril(ref, -1), 0), "U": (np.triu(ref), 1)}, {"rperm": rp, "rperm_inv": rpi, "cperm": cp, "cperm_inv": cpi, "count": nt}
    if family == "lblt":
        import lblt_ref

        r = lblt_ref.lblt_unblocked(a.astype(np.float64), case)
        return ({"L": (np.tril(r["L"], -1), 0), "D": (np.asarray(r["d"]), 1), "S": (np.asarray(r["subdiag"]), 1)},
                {"perm": np.asarray(r["perm_fwd"]), "count": r["transposition_count"], "npiv": list(r["npiv"])})
    if family == "piv_llt":
        import piv_llt_ref

        r = piv_llt_ref.piv_llt_unblocked(a.astype(np.float64))
        return {"L": (r["L"], 1)}, {"status": r["status"], "rank": r["rank"], "perm": np.asarray(r["perm_fwd"]), "count": r["transposition_count"]}
    raise KeyError(family)


def split_tridiag(v, h):
    n = v.shape[0]
    lo = np.zeros_like(v)
    il = np.tril_indices(n, -2)
    lo[il] = v[il]
    return {"T": (tridiag_of(v), 1), "V": (lo, 0), "H": (h, 0)}


def split_bidiag(u, hl, hr):
    if u.shape[0] >= u.shape[1]:
        b = bidiag_of(u)
    else:  # wide: min(m, n) rows; the last row is left normalised (svd/bidiag.rs:173-175), its entries right of the diagonal are O(1)
        b = np.zeros_like(u)
        for j in range(u.shape[0]):
            b[j, j] = u[j, j]
            if j + 1 < u.shape[0]:
                b[j, j + 1] = u[j, j + 1]
    return {"B": (b, 1), "V": (u - b, 0), "HL": (hl, 0), "HR": (hr, 0)}


def split_hessenberg(v, h):
    return {"HS": (hess_of(v), 1), "V": (np.tril(v, -2), 0), "H": (h, 0)}


def outputs_cap_ok(parts):
    return all(cap_ok_taus(x) for x, _ in parts.values())


# ------------------------------------------------------------------------------------------------ comparisons
# each works on unscaled fp64 parts `g` (got) and `r` (reference) and the UNSCALED input `a`: the bound of the family's existing oracle
# test, verbatim
def same_taus(h, ho, tol_of_column):
    fin = np.isfinite(ho)
    assert np.array_equal(np.isfinite(h), fin), "pattern of +inf taus"
    assert np.array_equal(h[~fin], ho[~fin])
    for j in range(ho.shape[1]):
        fj = fin[:, j]
        assert np.abs(h[fj, j] - ho[fj, j]).max(initial=0.0) <= tol_of_column(j), ("block factor column", j)


def compare_tridiag(g, r, a):
    """tests/test_gpu_tridiag.py::test_tridiag_vs_oracle"""
    n, eps = a.shape[0], EPS[a.dtype]
    scale = np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(g["T"] - r["T"]).max() <= 64 * n * eps * scale
    assert np.abs(g["V"] - r["V"]).max(initial=0.0) <= 64 * n * eps
    same_taus(g["H"], r["H"], lambda j: 64 * n * eps)


def compare_bidiag(g, r, a, bl=8, br=8):
    """tests/test_gpu_bidiag.py::test_bidiag_vs_oracle: B at 64 max(m, n) eps ||A||_2, every reflector and block factor column with the
    conditioning of the bidiagonal entry it produces"""
    m, n = a.shape
    eps, mx, size = EPS[a.dtype], max(m, n), min(m, n)
    scale = np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(g["B"] - r["B"]).max() <= 64 * mx * eps * scale
    bo = r["B"]
    dg, sg = np.abs(np.diag(bo))[:size], np.abs(np.diag(bo, 1))
    cl = np.maximum(1.0, scale / np.where(dg != 0, dg, scale))
    cr = np.maximum(1.0, scale / np.where(sg != 0, sg, scale))
    u, uo = g["V"], r["V"]
    for j in range(size):
        assert np.abs(u[j + 1:, j] - uo[j + 1:, j]).max(initial=0.0) <= 64 * mx * eps * cl[j], ("left", j)
        if j + 2 < n and j < len(cr):
            assert np.abs(u[j, j + 2:] - uo[j, j + 2:]).max(initial=0.0) <= 64 * mx * eps * cr[j], ("right", j)
    same_taus(g["HL"], r["HL"], lambda j: 64 * mx * eps * cl[(j // bl) * bl:j + 1].max(initial=1.0))
    same_taus(g["HR"], r["HR"], lambda j: 64 * mx * eps * cr[(j // br) * br:j + 1].max(initial=1.0))


def compare_hessenberg(g, r, a, b=8):
    """tests/test_gpu_hessenberg.py::_vs_oracle"""
    n, eps = a.shape[0], EPS[a.dtype]
    scale = np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(g["HS"] - r["HS"]).max() <= 64 * n * eps * scale
    sub = np.abs(np.diag(r["HS"], -1))
    cond = np.maximum(1.0, scale / np.where(sub != 0, sub, scale))
    v, vo = g["V"], r["V"]
    for j in range(n - 2):
        assert np.abs(v[j + 2:, j] - vo[j + 2:, j]).max(initial=0.0) <= 64 * n * eps * cond[j], j
    same_taus(g["H"], r["H"], lambda j: 64 * n * eps * cond[(j // b) * b:j + 1].max())


def compare_colpiv_qr(g, r, a, amax=None):
    """tests/test_gpu_qr.py::test_colpiv_qr_vs_oracle: 256 max(m, n) eps max(1, max |A|) for R and the reflectors, 4 times that for
    the block factors"""
    m, n = a.shape
    tol = 256 * max(m, n) * EPS[a.dtype] * max(1.0, np.abs(a).max() if amax is None else amax)
    assert np.abs(g["R"] - r["R"]).max() <= tol
    assert np.abs(g["V"] - r["V"]).max(initial=0.0) <= tol
    same_taus(g["H"], r["H"], lambda j: 4 * tol)


def compare_qr(g, r, a):
    """tests/test_gpu_qr.py::test_qr_norm_l2_scaling_cases"""
    m, n = a.shape
    size, eps = min(m, n), EPS[a.dtype]
    assert np.isfinite(g["R"]).all() and np.isfinite(g["V"]).all()
    assert np.abs(g["R"] - r["R"]).max() <= 512 * max(m, n) * eps * np.abs(r["R"]).max()
    assert np.abs(g["V"] - r["V"]).max(initial=0) <= 512 * max(m, n) * eps
    h, rh = g["H"], r["H"]
    tu = block_upper_mask(h.shape[0], size)
    fin = np.isfinite(rh)
    assert (np.isfinite(h) == fin).all()
    assert np.abs(np.where(fin, h, 0) - np.where(fin, rh, 0))[fin & tu].max(initial=0) <= 512 * max(m, n) * eps * max(1.0, np.abs(rh[fin & tu]).max(initial=0))


def compare_llt(g, r, a):
    """tests/test_gpu_factor.py::test_llt_vs_oracle"""
    n = a.shape[0]
    assert np.abs(np.tril(g["L"]) - np.tril(r["L"])).max() <= 64 * n * EPS[a.dtype] * np.abs(r["L"]).max()


def compare_ldlt(g, r, a):
    """tests/test_gpu_factor.py::test_ldlt_vs_oracle"""
    n = a.shape[0]
    got, ref = g["L"] + np.diag(g["D"]), r["L"] + np.diag(r["D"])
    assert np.abs(got - ref).max() <= 64 * n * EPS[a.dtype] * max(1.0, np.abs(ref).max())
    assert np.array_equal(np.sign(g["D"]), np.sign(r["D"]))


def compare_lu(g, r, a, perm=None):
    """tests/test_gpu_factor.py::test_plu_vs_oracle: 4 max(m, n) eps kappa max(1, max |LU|), kappa of the pivoted leading block"""
    m, n = a.shape
    size = min(m, n)
    kappa = np.linalg.cond(a[perm][:size, :size].astype(np.float64))
    got, ref = g["L"] + g["U"], r["L"] + r["U"]
    assert np.abs(got - ref).max() <= 4 * max(m, n) * EPS[a.dtype] * kappa * max(1.0, np.abs(ref).max())


def compare_fplu(g, r, a):
    """tests/test_gpu_factor.py::test_full_piv_lu_vs_oracle"""
    m, n = a.shape
    got, ref = g["L"] + g["U"], r["L"] + r["U"]
    assert np.abs(got - ref).max() <= 64 * max(m, n) * EPS[a.dtype] * max(1.0, np.abs(ref).max())


def compare_dense_sym(g, r, a):
    """tests/test_gpu_lblt.py / test_gpu_piv_llt.py: tol(n) = 64 n eps times max |A|, per stored factor"""
    n = a.shape[0]
    tol = 64 * max(n, 1) * EPS[a.dtype] * np.abs(a).max()
    for name in r:
        assert np.abs(g[name] - r[name]).max(initial=0.0) <= tol, name


COMPARE = {"tridiag": compare_tridiag, "bidiag": compare_bidiag, "hessenberg": compare_hessenberg, "colpiv_qr": compare_colpiv_qr,
           "qr": compare_qr, "llt": compare_llt, "ldlt": compare_ldlt, "fplu": compare_fplu, "lblt": compare_dense_sym,
           "piv_llt": compare_dense_sym}


def same_exact(x, y):
    assert x.keys() == y.keys()
    for k in x:
        if isinstance(x[k], np.ndarray):
            assert np.array_equal(x[k], y[k]), k
        else:
            assert x[k] == y[k], (k, x[k], y[k])


def family_cases(family):
    """(case, strategy-or-None) pairs: lblt runs every pivoting strategy it exposes"""
    if family == "lblt":
        import lblt_ref

        return [(c, s) for c in CASES[family] for s in lblt_ref.STRATEGIES]
    return [(c, None) for c in CASES[family]]
