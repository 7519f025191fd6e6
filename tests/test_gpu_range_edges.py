"""-m gpu: every factorization at the ends of the floating-point range.  The inputs, scale tables, references and bounds are those of
tests/range_cases.py (tests/test_range_cases.py shows, without a GPU, that the references themselves stay inside these bounds at
every scale used here): a kernel that restates the three-accumulator norm with `sml` and `big` swapped, squares an intermediate
or carries an absolute threshold the reference does not have fails here and nowhere else in the suite."""
import ctypes as C

import numpy as np
import pytest

import range_cases as rc
from gpu_util import EPS, bits, init_gpu, to_dev, to_host

pytestmark = pytest.mark.gpu

KIDX = [0, 1, 2, 3]  # (-extreme, -moderate, +moderate, +extreme) of rc.K[family][dtype]
KIDS = ["-extreme", "-moderate", "+moderate", "+extreme"]


def one_pass_columns(F):
    F.lib().faer_hip_debug_qr_one_pass_columns.restype = C.c_long
    return F.lib().faer_hip_debug_qr_one_pass_columns()


def gpu_factor(F, family, a, strat=None):
    """the device counterpart of rc.reference: ({part: (array, e)}, exact)"""
    dt = a.dtype
    if family == "tridiag":
        n = a.shape[0]
        vd, hd = to_dev(a), to_dev(np.zeros((8, n - 1), dtype=dt, order="F"))
        F.tridiag_in_place(vd, hd)
        v = np.array(to_host(vd))
        assert np.array_equal(bits(np.ascontiguousarray(v[np.triu_indices(n, 1)])), bits(np.ascontiguousarray(a[np.triu_indices(n, 1)]))), \
            "the strict upper triangle is never written"
        return rc.split_tridiag(v, np.array(to_host(hd))), {}
    if family == "bidiag":
        m, n = a.shape
        size = min(m, n)
        vd = to_dev(a)
        hl, hr = to_dev(np.zeros((8, size), dtype=dt, order="F")), to_dev(np.zeros((8, max(size - 1, 0)), dtype=dt, order="F"))
        F.bidiag_in_place(vd, hl, hr)
        return rc.split_bidiag(np.array(to_host(vd)), np.array(to_host(hl)), np.array(to_host(hr))), {}
    if family == "hessenberg":
        n = a.shape[0]
        vd, hd = to_dev(a), to_dev(np.zeros((8, n - 1), dtype=dt, order="F"))
        F.hessenberg_in_place(vd, hd)
        return rc.split_hessenberg(np.array(to_host(vd)), np.array(to_host(hd))), {}
    if family == "colpiv_qr":
        from oracle import oracle as O

        m, n = a.shape
        layout = "C" if a.flags.c_contiguous and not a.flags.f_contiguous else "F"
        da, dh = to_dev(a, layout), to_dev(np.zeros((O.qr_recommended_block_size(m, n, dt), min(m, n)), dtype=dt, order="F"))
        cf, cb, cnt = F.colpiv_qr_factor_in_place(da, dh)
        return rc.split_qr(np.array(to_host(da)), np.array(to_host(dh))), {"perm": cf.astype(np.int64), "perm_inv": cb.astype(np.int64), "count": cnt}
    if family == "qr":
        from oracle import oracle as O

        m, n = a.shape
        dqr, dh = to_dev(a), to_dev(np.zeros((rc.qr_block_size(O, m, n, dt), min(m, n)), dtype=dt, order="F"))
        rank = F.qr_factor_in_place(dqr, dh)
        return rc.split_qr(np.array(to_host(dqr)), np.array(to_host(dh))), {"rank": rank}
    if family == "llt":
        n = a.shape[0]
        marked = a.copy(order="F")
        marked[np.triu_indices(n, 1)] = -7.5
        d = to_dev(marked)
        assert F.llt_factor_in_place(d) == 0
        got = np.array(to_host(d))
        assert (got[np.triu_indices(n, 1)] == -7.5).all()
        return {"L": (np.tril(got), 1)}, {}
    if family == "ldlt":
        n = a.shape[0]
        marked = a.copy(order="F")
        marked[np.triu_indices(n, 1)] = -7.5
        d = to_dev(marked)
        cnt = F.ldlt_factor_in_place(d)
        got = np.array(to_host(d))
        assert (got[np.triu_indices(n, 1)] == -7.5).all()
        return {"L": (np.tril(got, -1), 0), "D": (np.diag(got).copy(), 2)}, {"status": ("ok", cnt)}
    if family == "lu":
        d = to_dev(a)
        p, pi, nt = F.partial_piv_lu_factor_in_place(d)
        lu = np.array(to_host(d))
        return {"L": (np.tril(lu, -1), 0), "U": (np.triu(lu), 1)}, {"perm": p.astype(np.int64), "perm_inv": pi.astype(np.int64), "count": nt}
    if family == "fplu":
        d = to_dev(a)
        rf, rb, cf, cb, cnt = F.full_piv_lu_factor_in_place(d)
        lu = np.array(to_host(d))
        return ({"L": (np.tril(lu, -1), 0), "U": (np.triu(lu), 1)},
                {"rperm": rf.astype(np.int64), "rperm_inv": rb.astype(np.int64), "cperm": cf.astype(np.int64), "cperm_inv": cb.astype(np.int64), "count": cnt})
    if family == "lblt":
        import test_gpu_lblt as tl

        r = tl.factor(F, a, strat)
        p = np.array(r["packed"])
        return ({"L": (np.tril(p, -1), 0), "D": (np.diag(p).copy(), 1), "S": (np.array(r["sub"]), 1)},
                {"perm": r["pf"].astype(np.int64), "count": r["count"], "last": tuple(r["last"])})
    if family == "piv_llt":
        import test_gpu_piv_llt as tp

        r = tp.factor(F, a)
        assert r["ok"]
        return {"L": (np.tril(np.array(r["packed"])), 1)}, {"rank": r["rank"], "perm": r["pf"].astype(np.int64), "count": r["count"], "last": tuple(r["last"])}
    raise KeyError(family)


def with_body(F, force, fn):
    F.lib().faer_hip_debug_level2_force_memory_bodies(force)
    try:
        return fn()
    finally:
        F.lib().faer_hip_debug_level2_force_memory_bodies(0)


# ------------------------------------------------------------------------------------------------ a. condensed forms
def invariants(family, g, a):
    """tests/test_gpu_level2_bodies.py: what a valid reduction keeps whatever signs its reflectors picked -- the spectrum (tridiagonal), the
    singular values (bidiagonal), the Frobenius norm and the trace (Hessenberg) -- on the unscaled condensed form"""
    eps, a64 = EPS[a.dtype], a.astype(np.float64)
    if family == "tridiag":
        from scipy.linalg import eigvalsh_tridiagonal

        n = a.shape[0]
        ev = np.linalg.eigvalsh(a64)
        t = g["T"]
        assert np.abs(eigvalsh_tridiagonal(np.diag(t).copy(), np.diag(t, -1).copy()) - ev).max() <= 64 * n * eps * np.abs(ev).max()
    elif family == "bidiag":
        m, n = a.shape
        size = min(m, n)
        sv = np.linalg.svd(a64, compute_uv=False)
        assert np.abs(np.linalg.svd(g["B"][:size, :size], compute_uv=False) - sv[:size]).max() <= 64 * max(m, n) * eps * sv[0]
    else:
        n = a.shape[0]
        fro, tr = np.linalg.norm(a64), np.trace(a64)
        assert abs(np.linalg.norm(g["HS"]) - fro) <= 64 * n * eps * fro
        assert abs(np.trace(g["HS"]) - tr) <= 64 * n * eps * fro


CONDENSED = [(f, c) for f in ("tridiag", "bidiag", "hessenberg") for c in rc.CASES[f]]


@pytest.mark.parametrize("ki", KIDX, ids=KIDS)
@pytest.mark.parametrize("force", [0, 1], ids=["registers", "memory"])
@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("family,case", CONDENSED, ids=[f"{f}-{c}".replace(" ", "") for f, c in CONDENSED])
def test_condensed_forms_vs_oracle(oracle, family, case, dtype, force, ki):
    """T / B / H within the bound of the family's oracle test times 2^k, reflectors and block factors within its O(1) bound, the oracle's
    pattern of +inf taus, in the register body and the memory-resident body of every vector kernel (csrc/condense.hip), in both types
    and entry by entry like the families' own oracle tests; on top of that the scaled invariants of tests/test_gpu_level2_bodies.py
    (spectrum, singular values, Frobenius norm and trace) where they cover the matrix (not a wide bidiagonalization)."""
    F = init_gpu()
    k = rc.K[family][np.dtype(dtype)][ki]
    a = rc.make_input(family, case, dtype)
    ak = rc.scaled(a, k)
    ref, _ = rc.reference(oracle, family, ak)
    got, _ = with_body(F, force, lambda: gpu_factor(F, family, ak))
    g, r = rc.unscaled_parts(got, k), rc.unscaled_parts(ref, k)
    for name in r:
        if name.startswith("H") and name != "HS":
            assert np.array_equal(np.isfinite(g[name]), np.isfinite(r[name])), name
        else:
            assert np.isfinite(g[name]).all(), name
    wide = family == "bidiag" and case[0] < case[1]
    rc.COMPARE[family](g, r, a)
    if not wide:
        invariants(family, g, a)


# ------------------------------------------------------------------------------------------------ b. QR with column pivoting
@pytest.mark.parametrize("ki", KIDX, ids=KIDS)
@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("case", rc.CASES["colpiv_qr"], ids=lambda c: "x".join(map(str, c)))
def test_colpiv_qr_vs_oracle(oracle, case, dtype, ki):
    """the oracle's permutation, transposition count and pattern of +inf taus; R within the bound of test_colpiv_qr_vs_oracle times 2^k,
    reflectors and block factors within its O(1) bound.  One case per restatement of the norm in csrc/colpiv_qr.hip (rc.CASES)."""
    F = init_gpu()
    k = rc.K["colpiv_qr"][np.dtype(dtype)][ki]
    a = rc.make_input("colpiv_qr", case, dtype)
    ak = rc.scaled(a, k)
    ref, xr = rc.reference(oracle, "colpiv_qr", ak)
    got, xg = gpu_factor(F, "colpiv_qr", ak)
    rc.same_exact(xr, xg)
    rc.compare_colpiv_qr(rc.unscaled_parts(got, k), rc.unscaled_parts(ref, k), a)


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_colpiv_qr_graded_columns(oracle, dtype):
    """columns scaled individually from 2^-kx to 2^kx (rc.GRADED_KX: the reference's own limit, it divides by the largest column norm
    first): scale_bwd = 1 / best is far from every other column, and the norms recomputed after a flush span the whole range.  Column
    norms differ by more than a factor of two: the oracle's permutation exactly.  Column j of R carries the scale of the column that
    was pivoted there: compared after dividing each column by it."""
    F = init_gpu()
    kx = rc.GRADED_KX[np.dtype(dtype)]
    a, g0, c = rc.graded_columns(300, 40, dtype, kx)
    ref, xr = rc.reference(oracle, "colpiv_qr", a)
    got, xg = gpu_factor(F, "colpiv_qr", a)
    rc.same_exact(xr, xg)
    cs = c[xr["perm"]][None, :]
    g = {n_: np.asarray(x, dtype=np.float64) / (cs if n_ == "R" else 1.0) for n_, (x, _) in got.items()}
    r = {n_: np.asarray(x, dtype=np.float64) / (cs if n_ == "R" else 1.0) for n_, (x, _) in ref.items()}
    rc.compare_colpiv_qr(g, r, g0)


# ------------------------------------------------------------------------------------------------ c. plain QR in fp32
def qr_fp32_expected_columns(case, ki):
    """the one-pass counter: n when the whole-matrix one-pass path took every column, 0 when it was tried and its range guard refused
    column 0, -1 when the shape is outside its rule (fewer than 1024 rows or fewer than 3 rows per column: the classic path)"""
    if case == (3000, 40):
        return 40 if ki in (1, 2) else 0  # 2^+-20 is inside TqLim<float>'s rms window [1e-12, 1e12], 2^-90 and 2^100 are not
    return -1


INNER_PANEL = [(300, 200), (1100, 400)]  # classic recursion whose leading 64-column panels have >= 256 rows and >= 4 rows per column


@pytest.mark.parametrize("ki", KIDX, ids=KIDS)
@pytest.mark.parametrize("case", rc.CASES["qr"], ids=lambda c: "x".join(map(str, c)))
def test_qr_fp32_vs_oracle(oracle, case, ki):
    """test_qr_norm_l2_scaling_cases in fp32, same rank / R / V / T bounds, the path pinned by the one-pass counter:
    (9, 10), (1023, 5), (42, 1): the cooperative leaf of the classic path alone (panels narrower than 16 columns);
    (3000, 40): the whole-matrix one-pass path at the moderate scales, refused by its range guard at the extreme ones (classic leaf);
    (300, 200), (1100, 400): the classic recursion, whose leading panels go to the one-pass panel (tsqr_panel_applicable) -- run with
    faer_hip_debug_qr_panels_one_pass on and off, both within the bound; at the moderate scales the two results differ, which shows
    that the inner panel ran (at the extreme ones its range guard hands the panel back to the leaf).
    The general path (the gq_* kernels) takes over only after a refusal of the leaf: test_qr_fp32_general_path_rank_deficient."""
    F = init_gpu()
    k = rc.K["qr"][rc.F32][ki]
    a = rc.make_input("qr", case, np.float32)
    ak = rc.scaled(a, k)
    ref, xr = rc.reference(oracle, "qr", ak)
    assert xr["rank"] == min(case)
    r = rc.unscaled_parts(ref, k)
    outs = []
    for on in ((1, 0) if case in INNER_PANEL else (1,)):
        F.lib().faer_hip_debug_qr_panels_one_pass(on)
        try:
            got, xg = gpu_factor(F, "qr", ak)
            cols = one_pass_columns(F)
        finally:
            F.lib().faer_hip_debug_qr_panels_one_pass(1)
        assert xg == xr
        assert cols == qr_fp32_expected_columns(case, ki), cols
        rc.compare_qr(rc.unscaled_parts(got, k), r, a)
        outs.append(got["R"][0] + got["V"][0])
    if len(outs) == 2 and ki in (1, 2):
        assert not np.array_equal(outs[0], outs[1]), "the one-pass panel inside the classic recursion did not run"


@pytest.mark.parametrize("ki", KIDX, ids=KIDS)
def test_qr_fp32_general_path_rank_deficient(oracle, ki):
    """the general path of the classic QR (gq_norms / gq_house / gq_dots / gq_heads / gq_update of csrc/qr.hip, which restate the
    three-accumulator norm literally) runs once the cooperative leaf has refused a column: a rank-deficient fp32 matrix, as in
    test_qr_classic_path_one_pass_panels_rank_deficient, at the scales of rc.K["qr_deficient"].  The oracle's rank, its pattern of skipped
    reflectors (tau = +inf) and Q R = A at that test's bound, relative to the scaled input."""
    from test_gpu_qr import q_from

    F = init_gpu()
    k = rc.K["qr_deficient"][rc.F32][ki]
    a = rc.rank_deficient(*rc.QR_DEFICIENT, np.float32)
    m, n = a.shape
    ak = rc.scaled(a, k)
    bs = 32
    ref, rh = ak.copy(order="F"), np.zeros((bs, n), dtype=np.float32, order="F")
    rk = oracle.qr_in_place(ref, rh)
    dqr, dh = to_dev(ak), to_dev(np.zeros((bs, n), dtype=np.float32))
    assert F.qr_factor_in_place(dqr, dh) == rk
    assert rc.QR_DEFICIENT[2] <= rk < n
    h = to_host(dh)
    assert np.array_equal(np.isinf(h), np.isinf(rh)) and not np.isnan(h).any()
    qr = to_host(dqr)
    assert np.isfinite(qr).all()
    q = q_from(F, dqr, dh, m, np.float32).astype(np.float64)
    R = rc.unscale(np.triu(qr), k, 1)
    assert np.abs(q @ R - a).max() <= 256 * np.sqrt(m) * EPS[rc.F32] * np.abs(a).max()


# ------------------------------------------------------------------------------------------------ d. the one-pass range guard
GUARD_SHAPE = (1024, 128)  # the smallest rows of the whole-matrix one-pass rule (1024 rows, 3 rows per column), two 64-column panels
GUARD_RMS = {rc.F32: (1e11, 1e-11, 1e13, 1e-13), rc.F64: (1e99, 1e-99, 1e101, 1e-101)}


def guard_case(dtype, rms, column):
    m, n = GUARD_SHAPE
    g = rc.rnd(np.random.default_rng(m + n), m, n, dtype)
    c = np.ones(n)
    if column is None:
        c[:] = rms
    else:
        c[column] = rms
    return np.asfortranarray(g * c[None, :].astype(dtype)), g, c


def classic_bound(F, oracle, a, g0, c, bs=64):
    """tests/test_gpu_qr.py::test_qr_classic_path_one_pass_panels_vs_oracle: 8 x 64 max(m, n) eps max(1, max |A|) for R (each column
    relative to its scale), V and T"""
    m, n = a.shape
    dt = a.dtype
    ref, rh = a.copy(order="F"), np.zeros((bs, n), dtype=dt, order="F")
    assert oracle.qr_in_place(ref, rh) == n
    dqr, dh = to_dev(a), to_dev(np.zeros((bs, n), dtype=dt))
    assert F.qr_factor_in_place(dqr, dh) == n
    cols = one_pass_columns(F)
    qr, h = to_host(dqr).astype(np.float64), to_host(dh).astype(np.float64)
    assert np.isfinite(qr).all() and np.isfinite(h).all()
    tol = 64 * max(m, n) * EPS[dt] * max(1.0, np.abs(g0).max())
    up = np.triu(np.ones((m, n), bool))
    d = np.abs(qr - ref)
    assert (np.where(up, d, 0) / c[None, :]).max() <= 8 * tol
    assert d[~up].max() <= 8 * tol
    tu = rc.block_upper_mask(bs, n)
    assert np.abs(h - rh)[tu].max() <= 8 * tol * max(1.0, np.abs(rh[tu]).max())
    return cols


@pytest.mark.parametrize("which", [0, 1], ids=["large", "small"])
@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_one_pass_guard_in_range(oracle, dtype, which):
    """rms 1e+-11 (fp32) / 1e+-99 (fp64), just inside TqLim's sq_lo / sq_hi: the whole factorization stays on the one-pass path and its
    factors are as good as at unit scale -- the claim the guard exists to make true"""
    import test_gpu_qr as tq
    import test_gpu_qr_f64_tall as tq64

    F = init_gpu()
    a, g0, c = guard_case(dtype, GUARD_RMS[np.dtype(dtype)][which], None)
    n = a.shape[1]
    if dtype == np.float32:
        dqr, dh, _, _ = tq._tall_vs_oracle(oracle, F, a, 64)
        tq._q_properties(F, dqr, dh, a)
    else:
        dqr, dh = tq64._vs_oracle(oracle, F, a, 64, expect_cols=n)
        tq64._q_properties(F, dqr, dh, a)
    # (both helpers assert that the one-pass counter equals n right after the factorization)


@pytest.mark.parametrize("which", [2, 3], ids=["large", "small"])
@pytest.mark.parametrize("column", [None, 5, 100], ids=["uniform", "first-panel", "later-panel"])
@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_one_pass_guard_out_of_range(oracle, dtype, column, which):
    """rms 1e+-13 (fp32) / 1e+-101 (fp64), just outside: the one-pass path takes no column (the guard looks at EVERY column before
    anything is written -- tq_panel_kernel, tq_y_kernel and tq_range_rest_kernel of csrc/tsqr.hip -- so no column is completed in front
    of a later panel either: the count is 0 for a bad column in the first panel and in a later one), the classic path factors the matrix
    within its bound of the oracle and nothing is non-finite"""
    F = init_gpu()
    a, g0, c = guard_case(dtype, GUARD_RMS[np.dtype(dtype)][which], column)
    assert classic_bound(F, oracle, a, g0, c) == 0


# ------------------------------------------------------------------------------------------------ e. Cholesky and LDLT
def llt_lookahead_env(F, monkeypatch, n):
    monkeypatch.setenv("FAER_HIP_LLT_LA_MIN", "2048")
    monkeypatch.setenv("FAER_HIP_LLT_TAIL", "0")
    F.lib().faer_hip_debug_llt_steps.restype = C.c_size_t
    codes = (C.c_int * (4 * 16))()
    assert F.lib().faer_hip_debug_llt_steps(*(C.c_size_t(v) for v in (n, 2048, 0, 8192, 8192)), codes, C.c_size_t(16)) >= 1


LLT_SIZES = rc.CASES["llt"] + [rc.LLT_LOOKAHEAD_N]


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("n", LLT_SIZES)
def test_llt_scaled_by_powers_of_four(n, dtype, monkeypatch):
    """the leaf, the blocked recursion and the look-ahead driver on A * 4^k against numpy's fp64 Cholesky of the rounded input times 2^k,
    at the bound of test_llt_vs_oracle.  fp64: the moderate k run the v_rsq_f64 chain of recip_sqrt, the extreme ones (pivots beyond
    1e+-280) its library fallback; the chain only sees the mantissa and the parity of the exponent, so within the moderate table
    L(A 4^k) == 2^k L(A) bit for bit."""
    F = init_gpu()
    if n == rc.LLT_LOOKAHEAD_N:
        llt_lookahead_env(F, monkeypatch, n)
    a = rc.make_input("llt", n, dtype)
    ref = np.linalg.cholesky(a.astype(np.float64))
    base = gpu_factor(F, "llt", a)[0]["L"][0]
    rc.compare_llt({"L": base.astype(np.float64)}, {"L": ref}, a)
    ks = rc.K["llt"][np.dtype(dtype)]
    for i, k in enumerate(ks):
        got = gpu_factor(F, "llt", rc.scaled(a, k, 2))[0]["L"][0]
        assert rc.cap_ok(got), k
        rc.compare_llt({"L": rc.unscale(got, k, 1)}, {"L": ref}, a)
        if dtype == np.float64 and i in (1, 2):
            assert np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(rc.scaled(base, k, 1)))), k


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("n", rc.CASES["ldlt"])
def test_ldlt_scaled_by_powers_of_four(oracle, n, dtype):
    """quasi-definite A * 4^k: unit L unchanged, D times 4^k, against the oracle at the bound of test_ldlt_vs_oracle; the signs of D.
    The leaf (n = 100) and the recursion by halves (n = 300) are all there is: LDLT has no look-ahead driver (potrf.hip runs
    chol_rec<T, true> at every size), and its pivots are divided by, never passed to recip_sqrt."""
    F = init_gpu()
    a = rc.make_input("ldlt", n, dtype)
    for k in rc.K["ldlt"][np.dtype(dtype)]:
        ak = rc.scaled(a, k, 2)
        ref, xr = rc.reference(oracle, "ldlt", ak)
        got, xg = gpu_factor(F, "ldlt", ak)
        assert xr == xg == {"status": ("ok", 0)}
        rc.compare_ldlt(rc.unscaled_parts(got, k), rc.unscaled_parts(ref, k), a)


@pytest.mark.parametrize("n,bad", [(100, 64), (300, 299)])
def test_llt_failure_index_at_extreme_scale(oracle, n, bad):
    """a diagonal entry turned negative mid-matrix (test_llt_non_positive_pivot): the same failing index at 4^+-480, where recip_sqrt's
    fallback branch decides, as at k = 0"""
    F = init_gpu()
    a = rc.spd(np.random.default_rng(7), n)
    a[bad, bad] = (a[bad, :bad] @ np.linalg.solve(a[:bad, :bad], a[:bad, bad])) - 1.0
    lo, _, _, hi = rc.K["llt"][rc.F64]
    for k in (0, lo, hi):
        ak = rc.scaled(a, k, 2)
        assert rc.cap_ok(ak)
        assert oracle.llt_in_place(ak.copy(order="F")) == ("non_positive_pivot", bad)
        with pytest.raises(F.LltError) as ei:
            F.llt_factor_in_place(to_dev(ak))
        assert ei.value.index == bad, k


# ------------------------------------------------------------------------------------------------ f. scale equivariance, bit for bit
EQUIVARIANT = [(f, c, s) for f in ("lu", "fplu", "lblt", "piv_llt") for c, s in rc.family_cases(f)]


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("family,case,strat", EQUIVARIANT, ids=[f"{f}-{c}-{s}".replace(" ", "") for f, c, s in EQUIVARIANT])
def test_pivoted_dense_factorizations_are_scale_equivariant(family, case, strat, dtype):
    """LU, full-pivot LU, lblt (every strategy) and piv_llt compute no norms: for A * 2^k (piv_llt: A * 4^k) the permutations, the
    transposition count, the status and the path counters are those of A and every stored factor is bit-identical to the factor of A
    with U / D / the subdiagonal (piv_llt: L) multiplied by 2^k.
    Thresholds that are legitimately absolute or relative and do not break this inside the tables: full-pivot LU skips a pivot whose
    score is below the smallest positive normal number (fplu.hip, like the reference) -- never reached by a full-rank Gaussian matrix
    whose scaled entries are normal; piv_llt's tolerance eps n max(diag) is relative and scales by 4^k exactly."""
    F = init_gpu()
    a = rc.make_input(family, case, dtype)
    e_in = rc.IN_EXP[family]
    base, xb = gpu_factor(F, family, a, strat)
    for k in rc.K[family][np.dtype(dtype)]:
        ak = rc.scaled(a, k, e_in)
        assert rc.cap_ok(ak)
        got, xg = gpu_factor(F, family, ak, strat)
        rc.same_exact(xb, xg)
        for name, (x, e) in base.items():
            want = rc.scaled(np.ascontiguousarray(x), k, e) if e else np.ascontiguousarray(x)
            have = np.ascontiguousarray(got[name][0])
            ne = bits(want) != bits(have)
            assert not ne.any(), (family, k, name, int(ne.sum()), tuple(np.argwhere(ne)[0]))
