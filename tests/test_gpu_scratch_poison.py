"""Every family on a poisoned scratch pool (faer_hip_debug_scratch_fill, csrc/ctx.hip).

All internal device memory comes from Ctx::alloc, which recycles buffers and never clears them: a kernel that reads scratch nothing
in the same call has written sees whatever the previous user left, on a fresh process very often zeros.  With the fill hook on, every
buffer the pool hands out is first filled over its whole pool size with one byte, stream ordered like the previous user's last write.
Each case builds its inputs once on the host and runs the same public call on fresh device copies with the fill off (twice: is the
path bitwise reproducible at all?), with 0xFF (NaN in both precisions, -1 in integers, every `>= epoch` flag already satisfied) and
with 0x7F (huge finite values, large positive integers), and asserts
  a. the outputs of the two filled runs, and of the unfilled one, are bitwise equal (paths found not reproducible without the hook
     print NOT-REPRODUCIBLE, drop this assertion and check both filled runs by (b));
  b. the 0xFF run passes the check of the family's existing test, whose tolerance expression is restated next to its name;
  c. nothing the call must not touch has changed (guard cells of tests/gpu_util.py, sentinel triangles, host parents), and the fill
     count of the call is > 0 -- or exactly 0 for the cases DESIGN.md ("Scratch sites") lists as allocation free.

SCRATCH_SITES is the per-file count of the objects that create scratch; tests/test_scratch_sites.py compares it with the sources, so a
new allocation site makes its author name the case that covers it here."""
import ctypes as C

import numpy as np
import pytest

from gpu_util import EPS, Routes, guard_intact, init_gpu, place_host, rnd, spd, to_dev, to_host, view_box
from test_bidiag_oracle import bidiag_of
from test_gpu_self_adjoint_evd import check as evd_check
from test_gpu_self_adjoint_evd import params as evd_params
from test_gpu_svd import check as svd_check
from test_gpu_svd import params as svd_params
from test_gpu_views import Held, block_upper, no_new_nan, q_from, quasi_definite, well_conditioned
from test_hessenberg_oracle import hess_of
from test_tridiag_oracle import tridiag_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]

# file under faer-rs_amd/csrc -> (scratch objects it creates: every declarator of a `Scratch` or `Staged<T>` declaration, every `.alloc(`,
# every optional<Scratch>, as tests/test_scratch_sites.py counts them; the tests that run the file's sites on a poisoned pool)
SCRATCH_SITES = {
    "api.hip": (91, "every test here with device operands passes through its Staged wrappers (no allocation: device pointers); "
                    "test_host_operands, test_cholesky_rebuild (wb / tb of reconstruct and inverse), test_pivoted_solves_and_rebuild"),
    "colpiv_qr.hip": (4, "test_colpiv_qr"),
    "common.h": (2, "Scratch and Staged themselves: every test here"),
    "condense.hip": (11, "test_tridiag, test_bidiag, test_hessenberg, test_self_adjoint_evd, test_svd"),
    "ctx.hip": (1, "the hop probe of faer_hip_xwg_hop_us clears its 512 bytes itself; a measurement aid, not on any product path"),
    "dist.hip": (1, "test_dist_single_rank"),
    "evd.hip": (8, "test_self_adjoint_evd"),
    "extras.hip": (2, "test_triangular_inverse, test_cholesky_rebuild"),
    "fplu.hip": (3, "test_full_piv_lu"),
    "gemm.hip": (2, "test_gemm_split_k (wsb); `out` of mfma_peak_tflops is a measurement aid"),
    "gemv.hip": (1, "test_gemv_sliced"),
    "getrf.hip": (12, "test_plu, test_plu_lookahead (listb, srcb, tmpb), test_plu_ties_and_zero_column, test_dist_single_rank"),
    "lblt.hip": (21, "test_lblt, test_host_operands (its Staged operands)"),
    "perm.h": (2, "test_pivoted_solves_and_rebuild, test_lblt, test_piv_llt"),
    "piv_llt.hip": (12, "test_piv_llt, test_host_operands (its Staged operands)"),
    "potrf.hip": (4, "test_llt_ldlt, test_ldlt_signs_and_regularization, test_llt_lookahead, test_llt_failure_then_success, test_dist_single_rank"),
    "qr.hip": (15, "test_qr_classic, test_qr_one_pass, test_qr_one_pass_falls_back_per_panel (h2), test_qr_rank_deficient (qr_general), test_colpiv_qr (T blocks)"),
    "skinny.hip": (1, "test_skinny_reduce"),
    "svd.hip": (17, "test_svd"),
    "trsm.hip": (1, "dead branch (prepack == false): test_trsm runs the live one and asserts it allocation free up to one block"),
    "tsqr.hip": (5, "test_qr_one_pass (panel copy on and off)"),
}

NOT_REPRODUCIBLE = []


@pytest.fixture
def fill():
    """fill(byte) switches the scratch fill on, fill(-1) off; always off again afterwards"""
    F = init_gpu()
    try:
        yield F.debug_scratch_fill
    finally:
        F.debug_scratch_fill(-1)


def same(x, y):
    """two output dicts, bit for bit"""
    if x.keys() != y.keys():
        return False
    for k in x:
        a, b = x[k], y[k]
        if isinstance(a, np.ndarray):
            if a.dtype != b.dtype or a.shape != b.shape or np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(b).tobytes():
                return False
        elif a != b:
            return False
    return True


def differing(x, y):
    return [k for k in x if not same({k: x[k]}, {k: y[k]})]


def poisoned(F, fill, call, check, what, alloc_free=False):
    """`call()` runs the public call on fresh copies of the inputs, asserts its guard cells and returns {name: output}"""
    fill(-1)
    base, again = call(), call()
    reproducible = same(base, again)
    fill(0xFF)
    ff = call()
    F.synchronize()
    count, nbytes = F.debug_scratch_fill_stats()
    fill(0x7F)
    sf = call()
    F.synchronize()
    fill(-1)
    print(f"scratch poison {what}: {count} fills, {nbytes} bytes, reproducible without the hook: {reproducible}")
    if alloc_free:
        assert count == 0, (what, count)
    else:
        assert count > 0 and nbytes >= 256 * count, (what, count, nbytes)
    check(ff)
    if reproducible:
        assert same(ff, sf), (what, "0xFF and 0x7F runs differ in", differing(ff, sf))
        assert same(ff, base), (what, "filled and unfilled runs differ in", differing(ff, base))
    else:
        NOT_REPRODUCIBLE.append(what)
        print(f"NOT-REPRODUCIBLE {what}: {differing(base, again)}")
        check(sf)


def sentinel_upper(a):
    m = a.copy()
    m[np.triu_indices(a.shape[0], 1)] = -7.5
    return m


# ------------------------------------------------------------------------------------------ GEMM split-K (gemm.hip wsb)
# DST_FULL splits from k = 1024 with fewer than 256 tiles (slices of >= 256, rounded up to 16): 64 x 64 x 1040 -> 4 slices of 272, the
# last one 224 long; 130 x 70 x 1030 -> several tiles, 4 slices of 272, last 214.  A lower destination splits from k = 4096 in slices
# of >= 1024: n = 200, k = 4100 -> 4 slices of 1040, last 980.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("accum", ["replace", "add"])
@pytest.mark.parametrize("kind,m,n,k", [("full", 64, 64, 1040), ("full", 130, 70, 1030), ("lower", 200, 200, 4100)])
def test_gemm_split_k(oracle, fill, kind, m, n, k, accum, dtype):
    F = init_gpu()
    rng = np.random.default_rng(m + n + k)
    a, b, c0 = rnd(rng, m, k, dtype), rnd(rng, k, n, dtype), rnd(rng, m, n, dtype)
    add = accum == "add"
    alpha = -0.5 if add else 2.0
    ref = c0.copy(order="F")
    oracle.matmul(ref, a, b, alpha=alpha, accum_add=add)
    lo = np.tril(np.ones((m, n), bool)) if kind == "lower" else np.ones((m, n), bool)
    # test_matmul_vs_oracle / test_gemm_inner_boundary_dst_kind (tests/test_gpu_matmul.py bound()): 4 K eps (|alpha| |A| |B| + |C0|)
    tol = 4 * k * EPS[np.dtype(dtype)] * (abs(alpha) * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)) + (np.abs(c0) if add else 0)) + 1e-300
    start = c0 if add else np.full((m, n), -7.5, dtype=dtype)

    def call():
        A, B, Cm = Held(a, "mat"), Held(b, "mat"), Held(start, "sub")
        with Routes(F) as r:
            F.gemm(Cm.view, F.DST_LOWER if kind == "lower" else F.DST_FULL, F.ACCUM_ADD if add else F.ACCUM_REPLACE, A.view, B.view, alpha)
        r.assert_hit("GemmSplitK")
        got = Cm.host()
        A.untouched("gemm lhs")
        B.untouched("gemm rhs")
        Cm.intact("gemm dst")
        assert np.array_equal(got[~lo], start[~lo]), "the strict upper triangle of a lower destination was written"
        return {"c": got}

    def check(o):
        assert np.isfinite(o["c"]).all()
        assert (np.abs(o["c"].astype(np.float64) - ref.astype(np.float64)) <= tol)[lo].all()

    poisoned(F, fill, call, check, f"gemm split-K {kind} {m}x{n}x{k} {accum} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ gemv slices, skinny reduce
# gemv.hip slices the reduction from k = 4096 when the rows fill fewer than 1024 workgroups, in slices rounded up to 256: k = 4096 ->
# 4 full slices; 4100 -> 4 slices of 1280, the last 260 long; 9000 -> 8 slices of 1280, the last 40 long
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["F", "C"])
def test_gemv_sliced(oracle, fill, order, dtype):
    F = init_gpu()
    for m in (1, 5, 300):
        for k in (4096, 4100, 9000):
            rng = np.random.default_rng(m * 7 + k)
            a, x, y0 = rnd(rng, m, k, dtype), rnd(rng, k, 1, dtype), rnd(rng, m, 1, dtype)
            for add, alpha in ((True, -0.5), (False, 2.0)):
                ref = y0.copy(order="F")
                oracle.matmul(ref, a, x, alpha=alpha, accum_add=add)
                # test_matmul_vs_oracle bound()
                tol = 4 * k * EPS[np.dtype(dtype)] * (abs(alpha) * (np.abs(a).astype(np.float64) @ np.abs(x).astype(np.float64)) + (np.abs(y0) if add else 0)) + 1e-300
                start = y0 if add else np.full((m, 1), -7.5, dtype=dtype)

                def call():
                    da, dx, Y = to_dev(a, order), to_dev(x), Held(start, "sub")
                    with Routes(F) as r:
                        F.matmul(Y.view, F.ACCUM_ADD if add else F.ACCUM_REPLACE, da, dx, alpha)
                    # (the level-2 stream; it has no counter of its own for the slices: with k >= 4096 and at most two row blocks
                    # the rule of gemv_dev gives k / 1024 >= 4 of them)
                    r.assert_hit("GemmGemv")
                    got = Y.host()
                    Y.intact("gemv y")
                    return {"y": got}

                def check(o):
                    assert np.isfinite(o["y"]).all()
                    assert (np.abs(o["y"].astype(np.float64) - ref.astype(np.float64)) <= tol).all()

                poisoned(F, fill, call, check, f"gemv {m}x{k} {order} add={add} {np.dtype(dtype).name}")


# skinny.hip reduce: m, n <= 16, k >= 256 (LONG), A with unit column stride, B with unit row stride; slices rounded up to 512:
# k = 1000 -> two slices, the last 488 long (7 x 9: ragged 8 x 8 blocks); k = 700 with 16 x 16
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,k", [(7, 9, 1000), (16, 16, 700)])
def test_skinny_reduce(oracle, fill, m, n, k, dtype):
    F = init_gpu()
    rng = np.random.default_rng(m + n + k)
    a, b, c0 = rnd(rng, m, k, dtype), rnd(rng, k, n, dtype), rnd(rng, m, n, dtype)
    for add, alpha in ((True, -0.5), (False, 2.0)):
        ref = c0.copy(order="F")
        oracle.matmul(ref, a, b, alpha=alpha, accum_add=add)
        tol = 4 * k * EPS[np.dtype(dtype)] * (abs(alpha) * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)) + (np.abs(c0) if add else 0)) + 1e-300
        start = c0 if add else np.full((m, n), -7.5, dtype=dtype)

        def call():
            da, db, Cm = to_dev(a, "C"), to_dev(b, "F"), Held(start, "mat")
            with Routes(F) as r:
                F.matmul(Cm.view, F.ACCUM_ADD if add else F.ACCUM_REPLACE, da, db, alpha)
            r.assert_hit("GemmSkinny")
            got = Cm.host()
            Cm.intact("skinny dst")
            return {"c": got}

        def check(o):
            assert np.isfinite(o["c"]).all()
            assert (np.abs(o["c"].astype(np.float64) - ref.astype(np.float64)) <= tol).all()

        poisoned(F, fill, call, check, f"skinny reduce {m}x{n}x{k} add={add} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ TRSM, triangular inverse
# n = 100: one 128-row leaf that packs its own triangle -- no scratch at all (the packed-image branch of trsm.hip is dead code);
# n = 129, 300: the recursion, whose products go through gemm_dev (which always takes its workspace slot)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("n,k", [(100, 5), (129, 3), (300, 200)])
def test_trsm(oracle, fill, n, k, unit, upper, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n * 31 + k)
    t = np.asarray(rnd(rng, n, n) / (n if unit else 1.0) + n * np.eye(n), dtype=dtype, order="F")
    b = rnd(rng, n, k, dtype)
    ref = b.copy(order="F")
    oracle.trsm(t, ref, upper=upper, unit=unit)
    fn = {(False, False): F.solve_lower_triangular_in_place, (True, False): F.solve_upper_triangular_in_place,
          (False, True): F.solve_unit_lower_triangular_in_place, (True, True): F.solve_unit_upper_triangular_in_place}[(upper, unit)]

    def call():
        T, X = Held(t, "mat"), Held(b, "sub")
        fn(T.view, X.view)
        got = X.host()
        T.untouched("trsm triangle")
        X.intact("trsm rhs")
        return {"x": got}

    def check(o):
        no_new_nan(o["x"], None, "trsm")
        # test_trsm
        assert np.abs(o["x"] - ref).max() <= 64 * n * EPS[np.dtype(dtype)] * max(1.0, np.abs(ref).max())

    poisoned(F, fill, call, check, f"trsm {n}x{k} unit={unit} upper={upper} {np.dtype(dtype).name}", alloc_free=n <= 128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("n", [129, 300])
def test_triangular_inverse(fill, n, unit, upper, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n * 4 + 2 * unit + upper)
    t = (rnd(rng, n, n, dtype) / n ** 0.5 + 2 * np.eye(n, dtype=dtype)).astype(dtype)
    tri = np.triu(t) if upper else np.tril(t)
    if unit:
        np.fill_diagonal(tri, 1.0)
    mask = (np.triu(np.ones((n, n), bool), 1 if unit else 0) if upper else np.tril(np.ones((n, n), bool), -1 if unit else 0))
    junk = t.copy() if not unit else t + 3 * np.eye(n, dtype=dtype)
    ref = np.linalg.inv(tri.astype(np.float64))

    def call():
        T, Out = Held(junk, "mat"), Held(np.full((n, n), -7.5, dtype=dtype), "sub")
        F.inverse_triangular_in_place(Out.view, T.view, upper=upper, unit=unit)
        got = Out.host()
        T.untouched("triangular inverse")
        Out.intact("triangular inverse")
        assert (got[~mask] == -7.5).all()
        return {"inv": got}

    def check(o):
        no_new_nan(o["inv"], None, "triangular inverse")
        # test_triangular_inverse (tests/test_gpu_extras.py tol(): 64 n eps)
        assert np.abs(o["inv"][mask] - ref[mask]).max(initial=0) <= 64 * n * EPS[np.dtype(dtype)] * max(1.0, np.abs(ref).max())

    poisoned(F, fill, call, check, f"triangular inverse {n} unit={unit} upper={upper} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ LLT, LDLT (potrf.hip)
# 31, 128: one leaf; 129, 300: blocked (packed images of the diagonal blocks in `winv`); LDLT adds `dv` / `sg`
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["llt", "ldlt"])
@pytest.mark.parametrize("n", [31, 128, 129, 300])
def test_llt_ldlt(oracle, fill, n, kind, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n)
    if kind == "llt":
        a = spd(rng, n, dtype)
    else:
        a, n1 = quasi_definite(rng, n, dtype)
    marked = sentinel_upper(a)
    ref = marked.copy(order="F")
    assert (oracle.llt_in_place if kind == "llt" else oracle.ldlt_in_place)(ref) == ("ok", 0)
    iu = np.triu_indices(n, 1)
    e = EPS[np.dtype(dtype)]

    def call():
        A = Held(marked, "sub")
        cnt = (F.llt_factor_in_place if kind == "llt" else F.ldlt_factor_in_place)(A.view)
        got = A.host()
        A.intact(kind)
        assert (got[iu] == -7.5).all(), "the strict upper triangle was written"
        return {"count": cnt, "factor": got}

    def check(o):
        got = o["factor"]
        assert o["count"] == 0
        no_new_nan(got, ref, kind)
        if kind == "llt":  # test_llt_vs_oracle
            L = np.tril(got).astype(np.float64)
            assert np.abs(np.tril(L @ L.T - a)).max() <= 8 * n * e * np.abs(a).max()
            assert np.abs(np.tril(got) - np.tril(ref)).max() <= 64 * n * e * np.abs(np.tril(ref)).max()
        else:  # test_ldlt_vs_oracle
            assert np.abs(np.tril(got) - np.tril(ref)).max() <= 64 * n * e * max(1.0, np.abs(np.tril(ref)).max())
            D = np.diag(got).astype(np.float64)
            assert (D[:n1] > 0).all() and (D[n1:] < 0).all()

    poisoned(F, fill, call, check, f"{kind} {n} {np.dtype(dtype).name}")


def test_ldlt_signs_and_regularization(oracle, fill):
    """test_ldlt_signs_and_regularization_on_views: a singular leading minor, regularized with the expected signs (the int8 signs are
    uploaded into scratch, `sg`)"""
    F = init_gpu()
    rng = np.random.default_rng(3)
    n, bad = 300, 211
    a, _ = quasi_definite(rng, n)
    sm = a.copy()
    sm[bad, :] = sm[5, :]
    sm[:, bad] = sm[:, 5]
    sm[bad, bad] = sm[5, 5]
    sm = sentinel_upper(sm)
    signs = np.where(np.arange(n) < n // 2, 1, -1).astype(np.int8)
    ref = sm.copy(order="F")
    rr = oracle.ldlt_in_place(ref, 1e-2, 1e-9, signs=signs)
    assert rr[0] == "ok"
    iu = np.triu_indices(n, 1)

    def call():
        A = Held(sm, "sub")
        cnt = F.ldlt_factor_in_place(A.view, (1e-2, 1e-9), signs=signs)
        got = A.host()
        A.intact("ldlt regularized")
        assert (got[iu] == -7.5).all()
        return {"count": cnt, "factor": got}

    def check(o):
        assert o["count"] == rr[1]
        no_new_nan(o["factor"], ref, "ldlt regularized")
        # test_ldlt_zero_pivot_regularization_and_solve
        assert np.abs(np.tril(o["factor"]) - np.tril(ref)).max() <= 1e-6 * max(1.0, np.abs(np.tril(ref)).max())

    poisoned(F, fill, call, check, "ldlt signs and regularization")


# the two-stream look-ahead driver through the plan knobs of test_llt_lookahead_path (LA_MIN = 2048, the smallest value that
# test uses, TAIL = 0): n = 2304 = 2048 + 2 x 128 is the size test_llt_lookahead_driver_on_views runs
@pytest.mark.parametrize("dtype", DTYPES)
def test_llt_lookahead(oracle, fill, dtype, monkeypatch):
    F = init_gpu()
    monkeypatch.setenv("FAER_HIP_LLT_LA_MIN", "2048")
    monkeypatch.setenv("FAER_HIP_LLT_TAIL", "0")
    n = 2304
    # the driver's own planning logic under the same knobs: at least one look-ahead step (n below LA_MIN has none and runs the recursion)
    F.lib().faer_hip_debug_llt_steps.restype = C.c_size_t
    codes = (C.c_int * (4 * 16))()
    assert F.lib().faer_hip_debug_llt_steps(*(C.c_size_t(v) for v in (n, 2048, 0, 8192, 8192)), codes, C.c_size_t(16)) >= 1
    a = spd(np.random.default_rng(77), n, dtype)
    marked = sentinel_upper(a)
    ref = marked.copy(order="F")
    assert oracle.llt_in_place(ref) == ("ok", 0)
    iu = np.triu_indices(n, 1)
    e = EPS[np.dtype(dtype)]

    def call():
        A = Held(marked, "mat")
        with Routes(F) as r:
            cnt = F.llt_factor_in_place(A.view)
        r.assert_hit("GemmTriEnum")  # the merged trailing updates of the blocked driver: square lower destinations
        got = A.host()
        A.intact("llt look-ahead")
        assert (got[iu] == -7.5).all()
        return {"count": cnt, "factor": got}

    def check(o):
        got = o["factor"]
        assert o["count"] == 0
        no_new_nan(got, ref, "llt look-ahead")
        L = np.tril(got).astype(np.float64)  # test_llt_vs_oracle
        assert np.abs(np.tril(L @ L.T - a)).max() <= 8 * n * e * np.abs(a).max()
        assert np.abs(np.tril(got) - np.tril(ref)).max() <= 64 * n * e * np.abs(np.tril(ref)).max()

    poisoned(F, fill, call, check, f"llt look-ahead {n} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["llt", "ldlt"])
def test_llt_failure_then_success(oracle, fill, kind, dtype):
    """a non-positive (LDLT: zero) pivot at a mid index, then a good matrix in the same process: the status words of the second
    call start clean (test_llt_non_positive_pivot_on_views, test_ldlt_zero_pivot_on_views)"""
    F = init_gpu()
    if kind == "llt":
        n, bad = 300, 211
        b = spd(np.random.default_rng(7), n, dtype)
        b[bad, bad] = -1.0
        expect, err = ("non_positive_pivot", bad), F.LltError
    else:
        n, bad = 150, 131
        rng = np.random.default_rng(5)
        Lm = np.tril(rng.integers(-1, 2, (n, n)), -1) * (rng.random((n, n)) < 0.1) + np.eye(n)
        d = rng.choice([1.0, 2.0, -1.0, -2.0], n)
        d[bad] = 0.0
        b = np.asarray((Lm * d) @ Lm.T, dtype=dtype)
        expect, err = ("zero_pivot", bad), F.LdltError
    bmark = sentinel_upper(b)
    rb = bmark.copy(order="F")
    assert (oracle.llt_in_place if kind == "llt" else oracle.ldlt_in_place)(rb) == expect
    good = spd(np.random.default_rng(8), n, dtype)
    gmark = sentinel_upper(good)
    ref = gmark.copy(order="F")
    assert (oracle.llt_in_place if kind == "llt" else oracle.ldlt_in_place)(ref) == ("ok", 0)
    fn = F.llt_factor_in_place if kind == "llt" else F.ldlt_factor_in_place
    iu = np.triu_indices(n, 1)

    def call():
        B, G = Held(bmark, "sub"), Held(gmark, "sub")
        with pytest.raises(err) as ei:
            fn(B.view)
        B.intact(kind + " failure")
        cnt = fn(G.view)
        got = G.host()
        G.intact(kind)
        assert (got[iu] == -7.5).all() and (B.host()[iu] == -7.5).all()
        return {"index": ei.value.index, "count": cnt, "factor": got}

    def check(o):
        assert o["index"] == bad and o["count"] == 0
        no_new_nan(o["factor"], ref, kind)
        # test_llt_vs_oracle / test_ldlt_vs_oracle
        assert np.abs(np.tril(o["factor"]) - np.tril(ref)).max() <= 64 * n * EPS[np.dtype(dtype)] * max(1.0, np.abs(np.tril(ref)).max())

    poisoned(F, fill, call, check, f"{kind} failure then success {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ partial-pivot LU (getrf.hip)
# (40, 17), (300, 8): single-workgroup leaf; (600, 5): cooperative leaf; (257, 257): recursion; (8, 300): wide; general = 1: every leaf
# on the non-cooperative path (pvb / prb / ub)
@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(40, 17), (300, 8), (600, 5), (257, 257), (8, 300)])
def test_plu(oracle, fill, m, n, dtype, general):
    F = init_gpu()
    a = rnd(np.random.default_rng(m * 7 + n), m, n, dtype)
    ref = a.copy(order="F")
    rperm, rinv, rnt = oracle.lu_in_place(ref)
    size = min(m, n)
    e = EPS[np.dtype(dtype)]

    def call():
        A = Held(a, "sub")
        F.lib().faer_hip_debug_lu_force_general(general)
        try:
            perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(A.view)
            lu = A.host()
        finally:
            F.lib().faer_hip_debug_lu_force_general(0)
        A.intact("lu")
        return {"lu": lu, "perm": perm, "perm_inv": perm_inv, "nt": nt}

    def check(o):
        lu, perm = o["lu"], o["perm"].astype(np.int64)
        no_new_nan(lu, ref, "lu")
        assert np.array_equal(perm, rperm) and np.array_equal(o["perm_inv"].astype(np.int64), rinv) and o["nt"] == rnt
        # test_plu_vs_oracle / test_plu_non_cooperative_leaves_vs_oracle
        L = (np.tril(lu[:, :size], -1) + np.eye(m, size)).astype(np.float64)
        U = np.triu(lu[:size, :]).astype(np.float64)
        assert np.abs(L @ U - a[perm]).max() <= 16 * max(m, n) * e * np.abs(a).max()
        assert np.abs(np.tril(lu, -1)).max(initial=0) <= 1.0 + 4 * e
        kappa = np.linalg.cond(a[perm][:size, :size].astype(np.float64))
        assert np.abs(lu - ref).max() <= 4 * max(m, n) * e * kappa * max(1.0, np.abs(ref).max())

    poisoned(F, fill, call, check, f"lu {m}x{n} general={general} {np.dtype(dtype).name}")


def test_plu_ties_and_zero_column(oracle, fill):
    """test_plu_ties_and_zero_column: an all-zero column (600 rows: cooperative leaf, 300 and 40: single-workgroup leaf) and ties
    between rows of different wavefronts"""
    F = init_gpu()
    inputs = []
    for rows in (600, 300, 40):
        z = np.zeros((rows, 5), order="F")
        z[:, 1:] = np.random.default_rng(3).standard_normal((rows, 4))
        inputs.append(z)
    t = np.random.default_rng(5).standard_normal((200, 6))
    t[150, 0] = t[20, 0] = -(np.abs(t[:, 0]).max() + 1.0)
    t[199, 2] = 9.0
    t[70, 2] = -9.0
    inputs.append(np.asfortranarray(t))
    for i, z in enumerate(inputs):
        ref = z.copy(order="F")
        rperm, _, _ = oracle.lu_in_place(ref)

        def call():
            A = Held(z, "mat")
            perm, _, _ = F.partial_piv_lu_factor_in_place(A.view)
            got = A.host()
            A.intact("lu")
            return {"lu": got, "perm": perm}

        def check(o):
            got = o["lu"]
            assert (o["perm"].astype(np.int64) == rperm).all()
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.allclose(got[~np.isnan(got)], ref[~np.isnan(ref)], rtol=1e-12, atol=1e-12)

        poisoned(F, fill, call, check, f"lu ties / zero column input {i}")


# look-ahead phases at small n as in test_plu_lookahead_phases_and_transitions_at_small_n: plan (512, 1536, 2048) at n = 3072 runs
# the pipelined, the plain bulk-bound and the staged steps (test_plu_lookahead_driver_on_views)
@pytest.mark.parametrize("dtype", DTYPES)
def test_plu_lookahead(oracle, fill, dtype):
    import torch

    F = init_gpu()
    n = 3072
    a = rnd(np.random.default_rng(n + 11), n, n, dtype)
    k = 256
    refp = a[:, :k].copy(order="F")
    rperm, _, _ = oracle.lu_in_place(refp)
    ad = torch.from_numpy(a).cuda()

    def call():
        A = Held(a, "mat")
        F.lib().faer_hip_debug_lu_plan(C.c_size_t(512), C.c_size_t(1536), C.c_size_t(2048))
        try:
            perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(A.view)
            F.synchronize()
        finally:
            F.lib().faer_hip_debug_lu_plan(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))
        A.intact("lu look-ahead")
        lu = A.view
        assert not torch.isnan(lu).any().item()
        p = torch.as_tensor(perm.astype(np.int64), device="cuda")
        Lm = (torch.tril(lu, -1) + torch.eye(n, dtype=lu.dtype, device="cuda")).double()
        U = torch.triu(lu).double()
        err = (Lm @ U - ad.double()[p]).abs().max().item()
        scale = (Lm.abs() @ U.abs()).max().item()
        return {"lu": A.host(), "perm": perm, "perm_inv": perm_inv, "nt": nt, "err": err, "scale": scale}

    def check(o):
        perm = o["perm"].astype(np.int64)
        assert sorted(perm.tolist()) == list(range(n)) and np.array_equal(o["perm_inv"].astype(np.int64)[perm], np.arange(n))
        assert np.array_equal(perm[:k], rperm[:k])
        if dtype == np.float64:  # test_plu_lookahead_phases_and_transitions_at_small_n
            assert o["err"] <= 16 * n * 2.3e-16 * o["scale"]
        else:  # test_lookahead_paths_fp32
            assert o["err"] <= 8 * n * 1.2e-7 * o["scale"]

    poisoned(F, fill, call, check, f"lu look-ahead {n} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ full-pivot LU (fplu.hip)
@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(40, 30), (30, 40), (300, 300)])
def test_full_piv_lu(oracle, fill, m, n, dtype, inplace):
    F = init_gpu()
    a = np.asarray(np.random.default_rng(m * 31 + n).standard_normal((m, n)), dtype=dtype)
    _, ref = place_host(a, "sub")
    rp, rpi, cp, cpi, nt = oracle.full_piv_lu_in_place(ref)

    def call():
        A = Held(a, "sub")
        F.lib().faer_hip_debug_fplu_inplace(inplace)
        try:
            rf, rb, cf, cb, cnt = F.full_piv_lu_factor_in_place(A.view)
            got = A.host()
        finally:
            F.lib().faer_hip_debug_fplu_inplace(0)
        A.intact("full-pivot lu")
        return {"lu": got, "rf": rf, "rb": rb, "cf": cf, "cb": cb, "nt": cnt}

    def check(o):
        no_new_nan(o["lu"], ref, "full-pivot lu")
        assert np.array_equal(o["rf"].astype(np.int64), rp) and np.array_equal(o["rb"].astype(np.int64), rpi)
        assert np.array_equal(o["cf"].astype(np.int64), cp) and np.array_equal(o["cb"].astype(np.int64), cpi) and o["nt"] == nt
        # test_full_piv_lu_vs_oracle
        assert np.abs(o["lu"] - ref).max() <= 64 * max(m, n) * EPS[np.dtype(dtype)] * max(1.0, np.abs(ref).max())

    poisoned(F, fill, call, check, f"full-pivot lu {m}x{n} inplace={inplace} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ QR (qr.hip, tsqr.hip)
def _qr_case(F, fill, oracle, a, bs, dtype, what, layout="sub", one_pass=None):
    m, n = a.shape
    size = min(m, n)
    _, ref = place_host(a, layout)
    _, rh = place_host(np.zeros((bs, size), dtype=dtype), layout)
    assert oracle.qr_in_place(ref, rh) == size
    e = EPS[np.dtype(dtype)]
    tol = 64 * max(m, n) * e * max(1.0, np.abs(a).max())
    F.lib().faer_hip_debug_qr_one_pass_columns.restype = C.c_long

    def call():
        A, H = Held(a, layout), Held(np.zeros((bs, size), dtype=dtype), layout)
        rank = F.qr_factor_in_place(A.view, H.view)
        if one_pass is not None:
            assert F.lib().faer_hip_debug_qr_one_pass_columns() == one_pass
        qr, h = A.host(), H.host()
        A.intact("qr")
        H.intact("qr coefficients")
        q = q_from(F, A.view[:, :size], H.view, m, dtype, layout)
        A.intact("qr basis read by the application")
        return {"rank": rank, "qr": qr, "h": h, "q": q}

    def check(o):
        qr, h, q = o["qr"], o["h"], o["q"].astype(np.float64)
        assert o["rank"] == size
        no_new_nan(qr, ref, "qr")
        no_new_nan(h, rh, "qr coefficients")
        # test_qr_full_rank_vs_oracle / test_qr_moderately_tall_one_pass_shape_rule
        assert np.abs(q @ np.triu(qr).astype(np.float64) - a).max() <= tol
        assert np.abs(q.T @ q - np.eye(m)).max() <= tol
        assert np.abs(qr.astype(np.float64) - ref).max() <= 8 * tol
        fin = np.isfinite(rh)
        assert (np.isfinite(h) == fin).all()
        up = block_upper(bs, size)
        assert np.abs(h.astype(np.float64) - np.where(fin, rh, 0.0))[fin & up].max(initial=0) <= 8 * tol * max(1.0, np.abs(rh[fin & up]).max(initial=0))

    poisoned(F, fill, call, check, what)


# the classic path: the cooperative panel kernel (flags, granules, slots, head, backup) with several block sizes of Q_coeff; `rowpad` has
# row stride != 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,bs,layout", [(100, 40, 4, "sub"), (40, 100, 15, "sub"), (512, 200, 32, "rowpad"), (300, 300, 48, "mat")])
def test_qr_classic(oracle, fill, capfd, m, n, bs, layout, dtype):
    F = init_gpu()
    a = rnd(np.random.default_rng(m * 131 + n), m, n, dtype)
    _qr_case(F, fill, oracle, a, bs, dtype, f"qr classic {m}x{n} bs={bs} {layout} {np.dtype(dtype).name}", layout, one_pass=-1)
    # full rank, so the only way onto the general path is the rerun after an exchange timeout, which the driver reports
    assert "timed out" not in capfd.readouterr().err, "the cooperative panel kernel did not run to its end: this case did not test it"


# the one-pass tall-skinny path, both precisions, at the smallest shape of its default rule (1024 rows, 3 rows per column: 1024 x 256
# is test_qr_moderately_tall_one_pass_shape_rule's first case; faer_hip_debug_qr_one_pass_shape_rule lowers the rule to 512 rows for
# the second shape), blocks of 48 (T rebuilt from V and the taus: `hown`), and without the panel copy (fp32)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,bs,copy,rule", [(1024, 256, 32, 1, None), (1024, 128, 48, 1, None), (1024, 256, 64, 0, None), (520, 70, 32, 1, (512, 3))])
def test_qr_one_pass(oracle, fill, m, n, bs, copy, rule, dtype):
    F = init_gpu()
    a = rnd(np.random.default_rng(m + 7 * n), m, n, dtype)
    F.lib().faer_hip_debug_qr_panel_copy(copy)
    if rule:
        F.lib().faer_hip_debug_qr_one_pass_shape_rule(C.c_long(rule[0]), C.c_long(rule[1]))
    try:
        _qr_case(F, fill, oracle, a, bs, dtype, f"qr one-pass {m}x{n} bs={bs} copy={copy} {np.dtype(dtype).name}", "mat", one_pass=n)
    finally:
        F.lib().faer_hip_debug_qr_panel_copy(1)
        F.lib().faer_hip_debug_qr_one_pass_shape_rule(C.c_long(0), C.c_long(0))


def _q_checks(F, oracle, a, bs, dtype, c, orth):
    """(call, check) of a QR whose factors are not compared entry by entry (an ill-conditioned or rank-deficient matrix): the oracle's
    rank and pattern of skipped reflectors, Q R == A and (orth) Q^T Q == I at c sqrt(m) eps"""
    m, n = a.shape
    size = min(m, n)
    ref, rh = a.copy(order="F"), np.zeros((bs, size), dtype=dtype, order="F")
    rk = oracle.qr_in_place(ref, rh)
    e = float(EPS[np.dtype(dtype)])
    F.lib().faer_hip_debug_qr_one_pass_columns.restype = C.c_long

    def call():
        A, H = Held(a, "mat"), Held(np.zeros((bs, size), dtype=dtype), "mat")
        rank = F.qr_factor_in_place(A.view, H.view)
        cols = F.lib().faer_hip_debug_qr_one_pass_columns()
        qr, h = A.host(), H.host()
        A.intact("qr")
        H.intact("qr coefficients")
        q = q_from(F, A.view[:, :size], H.view, m, dtype, "mat")
        return {"rank": rank, "cols": cols, "qr": qr, "h": h, "q": q}

    def check(o):
        assert o["rank"] == rk
        no_new_nan(o["qr"], ref, "qr")
        no_new_nan(o["h"], rh, "qr coefficients")
        assert np.array_equal(np.isinf(o["h"]), np.isinf(rh))
        q = o["q"].astype(np.float64)
        assert np.abs(q @ np.triu(o["qr"]).astype(np.float64) - a).max() <= c * np.sqrt(m) * e * np.abs(a).max()
        if orth:
            assert np.abs(q.T @ q - np.eye(m)).max() <= c * np.sqrt(m) * e

    return call, check, rk


# the per-panel fallback of test_qr_tall_falls_back_per_panel at 600 rows (faer_hip_debug_qr_one_pass_shape_rule lowers the 1024-row
# limit to 512): the first 64-column panel runs on the one-pass path, the second -- orthonormal columns times a Kahan-like triangle,
# cond ~ 1e5 against the guard's 512 (fp32) / 8 (fp64) -- is refused, and the classic path factors the rest from row and column 64
# (`h2`, geqrf_classic with an offset, the taus read back from its blocks, T rebuilt)
@pytest.mark.parametrize("dtype", DTYPES)
def test_qr_one_pass_falls_back_per_panel(oracle, fill, dtype):
    F = init_gpu()
    rng = np.random.default_rng(5)
    m, n = 600, 128
    a = rnd(rng, m, n, dtype)
    W = np.zeros((64, 64))
    W[0, 0] = 1.0
    for j in range(1, 64):
        W[:j, j] = -np.sqrt((1 - 0.75 ** 2) / j)
        W[j, j] = 0.75
    assert np.linalg.cond(W) > 2e4
    q2, _ = np.linalg.qr(rnd(rng, m, 64, np.float64))
    a[:, 64:128] = (q2 @ W * np.sqrt(m)).astype(dtype)
    # test_qr_tall_falls_back_per_panel: Q R == A and Q^T Q == I at 64 sqrt(m) eps
    call, check0, rk = _q_checks(F, oracle, a, 64, dtype, 64.0, True)
    assert rk == n

    def check(o):
        assert o["cols"] == 64, o["cols"]  # 0 < columns of the one-pass path < n: the first panel taken, the second refused
        check0(o)

    F.lib().faer_hip_debug_qr_one_pass_shape_rule(C.c_long(512), C.c_long(3))
    try:
        poisoned(F, fill, call, check, f"qr one-pass falls back per panel {np.dtype(dtype).name}")
    finally:
        F.lib().faer_hip_debug_qr_one_pass_shape_rule(C.c_long(0), C.c_long(0))


# a rank-deficient matrix on the classic path: the cooperative panel reports the dependent column and the factorization is redone
# from the saved copy on the general path (qr_general: `stb`, `dotsb` and its hand-sized memset, `kb`, `taus`)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,r,bs", [(100, 40, 10, 8), (300, 129, 50, 32)])
def test_qr_rank_deficient(oracle, fill, m, n, r, bs, dtype):
    F = init_gpu()
    rng = np.random.default_rng(21 + m)
    a = np.asfortranarray((rnd(rng, m, r) @ rnd(rng, r, n)).astype(dtype))
    # test_qr_classic_path_one_pass_panels_rank_deficient: the oracle's rank and +inf pattern, Q R == A at 256 sqrt(m) eps
    call, check0, rk = _q_checks(F, oracle, a, bs, dtype, 256.0, False)
    assert r <= rk < n

    def check(o):
        assert o["cols"] == -1
        check0(o)

    poisoned(F, fill, call, check, f"qr rank deficient {m}x{n} rank {r} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ column-pivot QR (colpiv_qr.hip)
# (200, 50), (30, 40): the register body; (4100, 8): more than 4096 rows, the memory body
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(30, 40), (200, 50), (4100, 8)])
def test_colpiv_qr(oracle, fill, m, n, dtype):
    F = init_gpu()
    a = np.asarray(np.random.default_rng(m * n).standard_normal((m, n)) * np.logspace(0, -3, n)[None, :], dtype=dtype)
    size = min(m, n)
    bs = oracle.qr_recommended_block_size(m, n, dtype)
    _, ref = place_host(a, "sub")
    _, href = place_host(np.zeros((bs, size), dtype=dtype), "sub")
    cp, cpi, nt = oracle.colpiv_qr_in_place(ref, href)

    def call():
        A, H = Held(a, "sub"), Held(np.zeros((bs, size), dtype=dtype), "sub")
        cf, cb, cnt = F.colpiv_qr_factor_in_place(A.view, H.view)
        got, hg = A.host(), H.host()
        A.intact("colpiv qr")
        H.intact("colpiv qr coefficients")
        return {"qr": got, "h": hg, "cf": cf, "cb": cb, "nt": cnt}

    def check(o):
        got, hg = o["qr"], o["h"]
        no_new_nan(got, ref, "colpiv qr")
        no_new_nan(hg, href, "colpiv qr coefficients")
        assert np.array_equal(o["cf"].astype(np.int64), cp) and np.array_equal(o["cb"].astype(np.int64), cpi) and o["nt"] == nt
        # test_colpiv_qr_vs_oracle
        tol = 256 * max(m, n) * EPS[np.dtype(dtype)] * max(1.0, np.abs(a).max())
        assert np.abs(got - ref).max() <= tol
        fin = np.isfinite(href)
        assert np.array_equal(np.isfinite(hg), fin) and np.array_equal(hg[~fin], href[~fin])
        assert np.abs(hg[fin] - href[fin]).max(initial=0) <= tol * 4

    poisoned(F, fill, call, check, f"colpiv qr {m}x{n} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ condensed forms (condense.hip)
class MemoryBodies:
    def __init__(self, F, on):
        self.lib, self.on = F.lib(), on

    def __enter__(self):
        self.lib.faer_hip_debug_level2_force_memory_bodies(self.on)

    def __exit__(self, *exc):
        self.lib.faer_hip_debug_level2_force_memory_bodies(0)
        return False


# (67, 4): odd, not divisible by the block; (129, 32): more than one 64-row tile block and one entry past a block of H
@pytest.mark.parametrize("mem", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", [(67, 4), (129, 32)])
def test_tridiag(fill, n, b, dtype, mem):
    from oracle import oracle as O

    F = init_gpu()
    x = np.random.default_rng(n * 7 + b).standard_normal((n, n))
    a = np.asarray(x + x.T, dtype=dtype)
    iu = np.triu_indices(n, 1)
    marked = sentinel_upper(a)
    _, vo = place_host(marked, "sub")
    _, ho = place_host(np.zeros((b, n - 1), dtype=dtype), "sub")
    O.tridiag_in_place(vo, ho)

    def call():
        A, H = Held(marked, "sub"), Held(np.zeros((b, n - 1), dtype=dtype), "sub")
        with MemoryBodies(F, mem):
            F.tridiag_in_place(A.view, H.view)
            v, h = A.host(), H.host()
        A.intact("tridiag")
        H.intact("tridiag coefficients")
        assert (v[iu] == -7.5).all()
        return {"v": v, "h": h}

    def check(o):
        v, h = o["v"], o["h"]
        no_new_nan(v, vo, "tridiag")
        no_new_nan(h, ho, "tridiag coefficients")
        # test_tridiag_vs_oracle
        eps = EPS[np.dtype(dtype)]
        scale = np.linalg.norm(a.astype(np.float64), 2)
        assert np.abs(tridiag_of(v) - tridiag_of(vo)).max() <= 64 * n * eps * scale
        il = np.tril_indices(n, -2)
        assert np.abs(v[il] - vo[il]).max(initial=0.0) <= 64 * n * eps
        fin = np.isfinite(ho)
        assert np.array_equal(np.isfinite(h), fin)
        assert np.abs(h[fin] - ho[fin]).max(initial=0.0) <= 64 * n * eps

    poisoned(F, fill, call, check, f"tridiag {n} b={b} mem={mem} {np.dtype(dtype).name}")


@pytest.mark.parametrize("mem", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,b", [(67, 4), (129, 32)])
def test_hessenberg(fill, n, b, dtype, mem):
    from oracle import oracle as O

    F = init_gpu()
    a = np.asarray(np.random.default_rng(n * 5 + b).standard_normal((n, n)), dtype=dtype)
    _, vo = place_host(a, "sub")
    _, ho = place_host(np.zeros((b, n - 1), dtype=dtype), "sub")
    O.hessenberg_in_place(vo, ho)

    def call():
        A, H = Held(a, "sub"), Held(np.zeros((b, n - 1), dtype=dtype), "sub")
        with MemoryBodies(F, mem):
            F.hessenberg_in_place(A.view, H.view)
            v, h = A.host(), H.host()
        A.intact("hessenberg")
        H.intact("hessenberg coefficients")
        return {"v": v, "h": h}

    def check(o):
        v, h = o["v"], o["h"]
        no_new_nan(v, vo, "hessenberg")
        no_new_nan(h, ho, "hessenberg coefficients")
        # test_hessenberg_vs_oracle
        eps = EPS[np.dtype(dtype)]
        scale = np.linalg.norm(a.astype(np.float64), 2)
        assert np.abs(hess_of(v) - hess_of(vo)).max() <= 64 * n * eps * scale
        sub = np.abs(np.diag(vo, -1)).astype(np.float64)
        cond = np.maximum(1.0, scale / np.where(sub != 0, sub, scale))
        for j in range(n - 2):
            assert np.abs(v[j + 2:, j] - vo[j + 2:, j]).max(initial=0.0) <= 64 * n * eps * cond[j], j
        fin = np.isfinite(ho)
        assert np.array_equal(np.isfinite(h), fin)
        for j in range(n - 1):
            cj = cond[(j // b) * b:j + 1].max()
            fj = fin[:, j]
            assert np.abs(h[fj, j] - ho[fj, j]).max(initial=0.0) <= 64 * n * eps * cj, j

    poisoned(F, fill, call, check, f"hessenberg {n} b={b} mem={mem} {np.dtype(dtype).name}")


# (130, 129): tall by one row; (67, 67): square -- the last column has no row below it (y2 = 0) -- and odd
@pytest.mark.parametrize("mem", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,bl,br", [(130, 129, 32, 16), (67, 67, 4, 4)])
def test_bidiag(fill, m, n, bl, br, dtype, mem):
    from oracle import oracle as O

    F = init_gpu()
    a = np.asarray(np.random.default_rng(m * 13 + n).standard_normal((m, n)), dtype=dtype)
    zl, zr = np.zeros((bl, n), dtype=dtype), np.zeros((br, n - 1), dtype=dtype)
    (_, uo), (_, hlo), (_, hro) = place_host(a, "sub"), place_host(zl, "sub"), place_host(zr, "sub")
    O.bidiag_in_place(uo, hlo, hro)

    def call():
        A, HL, HR = Held(a, "sub"), Held(zl, "sub"), Held(zr, "sub")
        with MemoryBodies(F, mem):
            F.bidiag_in_place(A.view, HL.view, HR.view)
            u, hl, hr = A.host(), HL.host(), HR.host()
        for held, what in ((A, "bidiag"), (HL, "bidiag left coefficients"), (HR, "bidiag right coefficients")):
            held.intact(what)
        return {"u": u, "hl": hl, "hr": hr}

    def check(o):
        u, hl, hr = o["u"], o["hl"], o["hr"]
        no_new_nan(u, uo, "bidiag")
        no_new_nan(hl, hlo, "bidiag left coefficients")
        no_new_nan(hr, hro, "bidiag right coefficients")
        # test_bidiag_vs_oracle
        eps = EPS[np.dtype(dtype)]
        scale = np.linalg.norm(a.astype(np.float64), 2)
        mx = max(m, n)
        assert np.abs(bidiag_of(u) - bidiag_of(uo)).max() <= 64 * mx * eps * scale
        bo = bidiag_of(uo).astype(np.float64)
        dg = np.abs(np.diag(bo))[:min(m, n)]
        sg = np.abs(np.diag(bo, 1))
        cl = np.maximum(1.0, scale / np.where(dg != 0, dg, scale))
        cr = np.maximum(1.0, scale / np.where(sg != 0, sg, scale))
        for j in range(min(m, n)):
            assert np.abs(u[j + 1:, j] - uo[j + 1:, j]).max(initial=0.0) <= 64 * mx * eps * cl[j], ("left", j)
            if j + 2 < n:
                assert np.abs(u[j, j + 2:] - uo[j, j + 2:]).max(initial=0.0) <= 64 * mx * eps * cr[j], ("right", j)
        for h, ho, cc, bb in ((hl, hlo, cl, bl), (hr, hro, cr, br)):
            fin = np.isfinite(ho)
            assert np.array_equal(np.isfinite(h), fin)
            for j in range(ho.shape[1]):
                cj = cc[(j // bb) * bb:j + 1].max(initial=1.0)
                fj = fin[:, j]
                assert np.abs(h[fj, j] - ho[fj, j]).max(initial=0.0) <= 64 * mx * eps * cj, j

    poisoned(F, fill, call, check, f"bidiag {m}x{n} mem={mem} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ self-adjoint EVD, SVD (evd.hip, svd.hip, dnc.h)
# n = 5 at the default recursion threshold 128: one leaf; n = 37 at threshold 4: at least two merge levels (leaves of at most 4 rows
# would need 10; whatever evd_leaf_size makes of 4, 37 rows are more than four leaves)
@pytest.mark.parametrize("with_u", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,rt", [(5, None), (37, 4), (130, 4)])
def test_self_adjoint_evd(fill, n, rt, dtype, with_u):
    import torch

    F = init_gpu()
    x = np.random.default_rng(n).standard_normal((n, n))
    a = np.asarray(x + x.T, dtype=dtype)
    marked = sentinel_upper(a)
    prm = evd_params(F, dtype, rt) if rt is not None else None
    tdt = torch.float64 if dtype == np.float64 else torch.float32

    def call():
        A = Held(marked, "sub")
        U = Held(np.zeros((n, n), dtype=dtype), "sub") if with_u else None
        s = torch.full((n,), -7.0, dtype=tdt, device="cuda")
        tag = F.self_adjoint_evd(A.view, s, U.view if with_u else None, prm)
        out = {"tag": tag, "s": to_host(s)}
        A.untouched("evd")
        if with_u:
            out["u"] = U.host()
            U.intact("evd eigenvectors")
        return out

    def check(o):
        assert o["tag"] == F.EVD_OK
        no_new_nan(o["s"], None, "eigenvalues")
        if with_u:
            no_new_nan(o["u"], None, "eigenvectors")
        evd_check(a, o["s"], o.get("u"))  # test_random_against_lapack: C_TOL n eps

    poisoned(F, fill, call, check, f"evd {n} rt={rt} vectors={with_u} {np.dtype(dtype).name}")


# (9, 7): one leaf; (41, 37) at recursion threshold 4: merge levels; (200, 20): m / n > 11 / 6, the QR pre-step
@pytest.mark.parametrize("vectors", ["thin", "no"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,rt", [(9, 7, None), (41, 37, 4), (200, 20, 4), (130, 130, 4)])
def test_svd(fill, m, n, rt, dtype, vectors):
    import torch

    F = init_gpu()
    a = np.asarray(np.random.default_rng(m * 3 + n).standard_normal((m, n)), dtype=dtype, order="F")
    k = min(m, n)
    prm = svd_params(F, dtype, rt)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    want = vectors == "thin"

    def call():
        A = Held(a, "sub")
        U = Held(np.full((m, k), -7.0, dtype=dtype), "sub") if want else None
        V = Held(np.full((n, k), -7.0, dtype=dtype), "sub") if want else None
        s = torch.full((k,), -7.0, dtype=tdt, device="cuda")
        tag = F.svd(A.view, s, U.view if want else None, V.view if want else None, prm)
        out = {"tag": tag, "s": to_host(s)}
        A.untouched("svd")
        if want:
            out["u"], out["v"] = U.host(), V.host()
            U.intact("svd u")
            V.intact("svd v")
        return out

    def check(o):
        assert o["tag"] == F.SVD_OK
        no_new_nan(o["s"], None, "singular values")
        svd_check(a, o["s"], o.get("u"), o.get("v"))  # test_random_shapes: C_TOL N eps

    poisoned(F, fill, call, check, f"svd {m}x{n} rt={rt} vectors={vectors} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["evd", "svd"])
def test_non_finite_then_good(fill, which, dtype):
    """test_non_finite_input_is_no_convergence followed by a good call: the status block of the second call starts clean"""
    import torch

    F = init_gpu()
    n = 37
    x = np.random.default_rng(n + 1).standard_normal((n, n))
    good = np.asarray(x + x.T, dtype=dtype, order="F")
    bad = good.copy()
    bad[n // 2, n // 3] = bad[n // 3, n // 2] = np.nan
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    prm = evd_params(F, dtype, 4) if which == "evd" else svd_params(F, dtype, 4)

    def one(mat):
        A, U = Held(mat, "sub"), Held(np.zeros((n, n), dtype=dtype), "sub")
        s = torch.full((n,), -7.0, dtype=tdt, device="cuda")
        if which == "evd":
            tag = F.self_adjoint_evd(A.view, s, U.view, prm)
            V = None
        else:
            V = Held(np.zeros((n, n), dtype=dtype), "sub")
            tag = F.svd(A.view, s, U.view, V.view, prm)
            V.intact("v")
        A.untouched("a")
        U.intact("u")
        return tag, to_host(s), U.host(), (V.host() if V else None)

    def call():
        tag_bad = one(bad)[0]
        tag, s, u, v = one(good)
        out = {"tag_bad": tag_bad, "tag": tag, "s": s, "u": u}
        if v is not None:
            out["v"] = v
        return out

    def check(o):
        assert o["tag_bad"] == (F.EVD_NO_CONVERGENCE if which == "evd" else F.SVD_NO_CONVERGENCE)
        assert o["tag"] == 0
        if which == "evd":
            evd_check(good, o["s"], o["u"])
        else:
            svd_check(good, o["s"], o["u"], o["v"])

    poisoned(F, fill, call, check, f"{which} non-finite then good {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ lblt, piv_llt (+ perm.h)
# n = 40: the leaf alone (n <= 64); n = 130 = 2 * 64 + 2: two panels and a leaf
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strat", ["partial_diag", "rook"])
@pytest.mark.parametrize("n", [40, 130])
def test_lblt(fill, n, strat, dtype):
    import lblt_ref as ref

    F = init_gpu()
    a = np.asarray(ref.random_symmetric(n, 1000 + n), dtype=dtype)
    a64 = a.astype(np.float64)
    marked = sentinel_upper(a)
    bs = {k: np.asarray(np.random.default_rng(n + k).standard_normal((n, k)), dtype=dtype, order="F") for k in (1, 129)}
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)
    t = 64 * n * EPS[np.dtype(dtype)]  # tests/test_gpu_lblt.py tol()

    def call():
        import torch

        A = Held(marked, "sub")
        sub = torch.zeros(n, dtype=A.view.dtype, device="cuda")
        _, pf, pb, cnt = F.lblt_factor_in_place(A.view, subdiag=sub, pivoting=ref.STRATEGIES[strat][0])
        packed = A.host()
        A.intact("lblt")
        assert (packed[iu] == -7.5).all()
        out = {"packed": packed, "sub": to_host(sub), "pf": pf, "pb": pb, "count": cnt}
        for k, b in bs.items():
            X = Held(b, "sub")
            F.lblt_solve_in_place(A.view, sub, pf, pb, X.view)
            out[f"x{k}"] = X.host()
            X.intact("lblt solve")
        R, Inv = Held(np.full((n, n), -7.5, dtype=dtype), "sub"), Held(np.full((n, n), -7.5, dtype=dtype), "sub")
        F.lblt_reconstruct(R.view, A.view, sub, pf, pb)
        F.lblt_inverse(Inv.view, A.view, sub, pf, pb)
        out["rec"], out["inv"] = R.host(), Inv.host()
        Eye = Held(np.eye(n, dtype=dtype), "sub")
        F.lblt_solve_in_place(A.view, sub, pf, pb, Eye.view)
        out["eye"] = Eye.host()
        Eye.intact("lblt solve on the identity")
        R.intact("lblt reconstruct")
        Inv.intact("lblt inverse")
        assert (out["rec"][iu] == -7.5).all()
        A.intact("lblt factors read")
        return out

    def check(o):
        amax = np.abs(a).max()
        p = o["packed"].astype(np.float64)
        pf = o["pf"].astype(np.int64)
        assert sorted(pf) == list(range(n)) and np.array_equal(pf[o["pb"].astype(np.int64)], np.arange(n))
        L = ref.unit_lower(p)
        # check_accuracy
        assert np.abs(a64[np.ix_(pf, pf)] - L @ ref.block_diag(np.diag(p), o["sub"].astype(np.float64)) @ L.T).max() <= t * amax
        assert np.abs(o["rec"][il].astype(np.float64) - a[il]).max() <= t * amax
        # check_solve
        for k, b in bs.items():
            xs = o[f"x{k}"].astype(np.float64)
            assert np.linalg.norm(a64 @ xs - b) <= t * np.linalg.norm(a64) * np.linalg.norm(xs), (k,)
        no_new_nan(o["inv"], None, "lblt inverse")
        # check_solve: the inverse is the solve on the identity, bit for bit
        assert same({"inv": o["inv"]}, {"inv": o["eye"]})

    poisoned(F, fill, call, check, f"lblt {n} {strat} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,kind", [(40, "spd"), (130, "spd"), (130, "low_rank")])
def test_piv_llt(fill, n, kind, dtype):
    import piv_llt_ref as ref

    F = init_gpu()
    a = np.asarray((ref.spd if kind == "spd" else ref.low_rank)(n, 1000 + n), dtype=dtype)
    a64 = a.astype(np.float64)
    marked = sentinel_upper(a)
    bs = {k: np.asarray(np.random.default_rng(n + k).standard_normal((n, k)), dtype=dtype, order="F") for k in (1, 129)}
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)
    t = 64 * n * EPS[np.dtype(dtype)]  # tests/test_gpu_piv_llt.py tol()

    def call():
        A = Held(marked, "sub")
        st = F.piv_llt_factor_in_place(A.view, raise_on_error=False)
        packed = A.host()
        A.intact("piv_llt")
        assert (packed[iu] == -7.5).all()
        if not isinstance(st, tuple):
            return {"packed": packed, "tag": st.tag, "index": st.index}
        pf, pb, rank, cnt = st
        out = {"packed": packed, "pf": pf, "pb": pb, "rank": rank, "count": cnt}
        R = Held(np.full((n, n), -7.5, dtype=dtype), "sub")
        F.piv_llt_reconstruct(R.view, A.view, pf, pb)
        out["rec"] = R.host()
        R.intact("piv_llt reconstruct")
        assert (out["rec"][iu] == -7.5).all()
        if kind == "spd":
            for k, b in bs.items():
                X = Held(b, "sub")
                F.piv_llt_solve_in_place(A.view, pf, pb, X.view)
                out[f"x{k}"] = X.host()
                X.intact("piv_llt solve")
            Inv = Held(np.full((n, n), -7.5, dtype=dtype), "sub")
            F.piv_llt_inverse(Inv.view, A.view, pf, pb)
            out["inv"] = Inv.host()
            Inv.intact("piv_llt inverse")
            assert (out["inv"][iu] == -7.5).all()
        return out

    def check(o):
        assert "pf" in o, o
        amax = np.abs(a64).max()
        pf = o["pf"].astype(np.int64)
        assert sorted(pf) == list(range(n)) and np.array_equal(pf[o["pb"].astype(np.int64)], np.arange(n))
        rank = o["rank"]
        if kind == "spd":
            assert rank == n
        else:
            assert 0 < rank < n
        L = np.tril(o["packed"].astype(np.float64))[:, :rank]
        # test_spd / test_pivot_parity_low_rank: the residual of the first `rank` columns
        assert np.abs(a64[np.ix_(pf, pf)] - L @ L.T).max() <= t * amax
        if kind == "spd":
            assert np.abs(o["rec"][il].astype(np.float64) - a64[il]).max() <= t * amax
            for k, b in bs.items():
                xs = o[f"x{k}"].astype(np.float64)
                assert np.linalg.norm(a64 @ xs - b) <= t * np.linalg.norm(a64) * np.linalg.norm(xs), (k,)
            ginv = o["inv"].astype(np.float64)
            sinv = np.linalg.inv(a64)
            # test_spd: against another inverse at n eps cond(A) max |A^-1|
            assert np.abs(ginv[il] - sinv[il]).max() <= t * np.abs(sinv).max() * np.linalg.cond(a64)

    poisoned(F, fill, call, check, f"piv_llt {n} {kind} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ permuted solves and rebuilds (perm.h)
# k = 1 and k = 129: one right-hand side, and one more than a 128-wide block
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["lu", "full_piv_lu", "colpiv_qr"])
@pytest.mark.parametrize("n", [130])
def test_pivoted_solves_and_rebuild(fill, n, kind, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n * 3 + len(kind))
    a = well_conditioned(rng, n, dtype)
    a64 = a.astype(np.float64)
    bs = {k: rnd(rng, n, k, dtype) for k in (1, 129)}
    e = EPS[np.dtype(dtype)]

    def call():
        A = Held(a, "sub")
        out = {}
        if kind == "lu":
            pf, pb, _ = F.partial_piv_lu_factor_in_place(A.view)
            solve = lambda X, tr: F.partial_piv_lu_solve_in_place(A.view, pf, pb, X, transpose=tr)
            rec = lambda o: F.partial_piv_lu_reconstruct(o, A.view, pf, pb)
            inv = lambda o: F.partial_piv_lu_inverse(o, A.view, pf, pb)
            out["pf"] = pf
        elif kind == "full_piv_lu":
            rf, rb, cf, cb, _ = F.full_piv_lu_factor_in_place(A.view)
            solve = lambda X, tr: F.full_piv_lu_solve_in_place(A.view, rf, rb, cf, cb, X, transpose=tr)
            rec = lambda o: F.full_piv_lu_reconstruct(o, A.view, rf, rb, cf, cb)
            inv = lambda o: F.full_piv_lu_inverse(o, A.view, rf, rb, cf, cb)
            out["rf"], out["cf"] = rf, cf
        else:
            bsz = F.qr_recommended_block_size(n, n, dtype)
            H = Held(np.zeros((bsz, n), dtype=dtype), "sub")
            cf, cb, _ = F.colpiv_qr_factor_in_place(A.view, H.view)
            H.intact("colpiv qr coefficients")
            solve = lambda X, tr: F.colpiv_qr_solve_in_place(A.view, H.view, cf, cb, X, mode="transpose" if tr else "solve")
            rec = lambda o: F.colpiv_qr_reconstruct(o, A.view, H.view, cf, cb)
            inv = lambda o: F.colpiv_qr_inverse(o, A.view, H.view, cf, cb)
            out["cf"] = cf
        A.intact(kind)
        for k, b in bs.items():
            for tr in (False, True):
                X = Held(b, "sub")
                solve(X.view, tr)
                out[f"x{k}{'t' if tr else ''}"] = X.host()
                X.intact(kind + " solve")
        R, Inv = Held(np.full((n, n), np.nan, dtype=dtype), "sub"), Held(np.full((n, n), np.nan, dtype=dtype), "sub")
        rec(R.view)
        inv(Inv.view)
        out["rec"], out["inv"] = R.host(), Inv.host()
        R.intact(kind + " reconstruct")
        Inv.intact(kind + " inverse")
        A.intact(kind + " factors read")
        return out

    def check(o):
        kappa = np.linalg.cond(a64)
        for k, b in bs.items():
            for tr in (False, True):
                x = o[f"x{k}{'t' if tr else ''}"]
                no_new_nan(x, None, kind + " solve")
                if kind == "full_piv_lu":  # test_full_piv_lu_vs_oracle: the residual of the solve and of the transpose solve
                    assert np.abs((a64.T if tr else a64) @ x - b).max() <= 256 * n * e * kappa * np.abs(b).max()
                else:
                    # test_partial_piv_lu_solve_vs_oracle / test_colpiv_qr_index_types_and_solve_modes (solve_tol): the forward
                    # error 64 n eps cond max(1, |ref|), here against the fp64 solution
                    ref = np.linalg.solve(a64.T if tr else a64, b.astype(np.float64))
                    assert np.abs(x.astype(np.float64) - ref).max() <= 64 * n * e * kappa * max(1.0, np.abs(ref).max())
        no_new_nan(o["rec"], None, kind + " reconstruct")
        no_new_nan(o["inv"], None, kind + " inverse")
        # test_lu_reconstruct_and_inverse and its siblings (tests/test_gpu_extras.py tol())
        assert np.abs(o["rec"] - a).max() <= 64 * n * e * np.abs(a).max()
        assert np.abs(o["inv"].astype(np.float64) @ a64 - np.eye(n)).max() <= 256 * n * e * kappa

    poisoned(F, fill, call, check, f"{kind} solves and rebuild {n} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["llt", "ldlt"])
@pytest.mark.parametrize("n", [129, 300])
def test_cholesky_rebuild(fill, n, kind, dtype):
    """test_llt_reconstruct_and_inverse / test_ldlt_reconstruct_and_inverse, and the solve"""
    F = init_gpu()
    rng = np.random.default_rng(n + (kind == "ldlt"))
    a = spd(rng, n, dtype)
    a64 = a.astype(np.float64)
    b = rnd(rng, n, 9, dtype)
    marked = sentinel_upper(a)
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)
    e = EPS[np.dtype(dtype)]

    def call():
        A = Held(marked, "sub")
        assert (F.llt_factor_in_place if kind == "llt" else F.ldlt_factor_in_place)(A.view) == 0
        R, Inv, X = Held(np.full((n, n), -7.5, dtype=dtype), "sub"), Held(np.full((n, n), -7.5, dtype=dtype), "sub"), Held(b, "sub")
        (F.llt_reconstruct if kind == "llt" else F.ldlt_reconstruct)(R.view, A.view)
        (F.llt_inverse if kind == "llt" else F.ldlt_inverse)(Inv.view, A.view)
        (F.llt_solve_in_place if kind == "llt" else F.ldlt_solve_in_place)(A.view, X.view)
        out = {"rec": R.host(), "inv": Inv.host(), "x": X.host()}
        for h in (A, R, Inv, X):
            h.intact(kind)
        assert (out["rec"][iu] == -7.5).all() and (out["inv"][iu] == -7.5).all()
        return out

    def check(o):
        for v in o.values():
            no_new_nan(v, None, kind)
        assert np.abs(o["rec"][il] - a[il]).max() <= 64 * n * e * np.abs(a).max()
        g = o["inv"].astype(np.float64)
        ainv = np.tril(g) + np.tril(g, -1).T
        assert np.abs(ainv @ a64 - np.eye(n)).max() <= 256 * n * e * np.linalg.cond(a64)
        ref = np.linalg.solve(a64, b.astype(np.float64))
        # test_llt_solve_vs_oracle
        assert np.abs(o["x"].astype(np.float64) - ref).max() <= 64 * n * e * np.linalg.cond(a64) * max(1.0, np.abs(ref).max())

    poisoned(F, fill, call, check, f"{kind} rebuild {n} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ host operands (Staged, common.h)
class HostHeld:
    """a numpy matrix inside a guarded host parent (place_host): a strided sub-view with NaN-patterned cells around it"""

    def __init__(self, a, layout="sub"):
        a = np.asarray(a)
        self.parent, self.view = place_host(a, layout)
        self.before = self.parent.copy()
        self.box = view_box(a.shape, layout, a.dtype)

    def intact(self, what=""):
        guard_intact(self.parent, self.before, self.box, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", ["matmul", "gemv", "trsm", "triangular_inverse", "llt", "ldlt", "lu", "qr", "svd", "evd", "lblt", "piv_llt",
                                    "full_piv_lu", "colpiv_qr", "tridiag", "bidiag", "hessenberg"])
def test_host_operands(fill, family, dtype):
    """host pointers on strided sub-views; the outputs that the boundary stages without copy-in (SVD u / v / s, reconstruct and
    inverse `out`, the Householder coefficient matrix) must come back fully written: no NaN inside the view, the parent untouched"""
    F = init_gpu()
    n = 70
    rng = np.random.default_rng(n + len(family))
    e = EPS[np.dtype(dtype)]
    nanm = lambda r, c: np.full((r, c), np.nan, dtype=dtype)
    a = well_conditioned(rng, n, dtype)
    s_a = spd(rng, n, dtype)
    a64, s64 = a.astype(np.float64), s_a.astype(np.float64)

    def finish(out, held):
        for h in held:
            h.intact(family)
        return out

    def call():
        if family == "matmul":  # split-K through staged operands
            x, y = rnd(np.random.default_rng(1), 64, 1040, dtype), rnd(np.random.default_rng(2), 1040, 64, dtype)
            X, Y, Z = HostHeld(x), HostHeld(y), HostHeld(nanm(64, 64))
            F.matmul(Z.view, F.ACCUM_REPLACE, X.view, Y.view, 1.0)
            return finish({"c": Z.view.copy(), "ref": x.astype(np.float64) @ y.astype(np.float64),
                           "absprod": np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64)}, [X, Y, Z])
        if family == "gemv":  # the sliced reduction (k = 4100: four slices, the last 260 long) through staged operands
            x, y = rnd(np.random.default_rng(1), 5, 4100, dtype), rnd(np.random.default_rng(2), 4100, 1, dtype)
            X, Y, Z = HostHeld(x), HostHeld(y), HostHeld(nanm(5, 1))
            F.matmul(Z.view, F.ACCUM_REPLACE, X.view, Y.view, 1.0)
            return finish({"c": Z.view.copy(), "ref": x.astype(np.float64) @ y.astype(np.float64),
                           "absprod": np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64)}, [X, Y, Z])
        if family == "trsm":
            nt = 129
            t = np.asarray(rnd(np.random.default_rng(4), nt, nt) + nt * np.eye(nt), dtype=dtype, order="F")
            b = rnd(np.random.default_rng(5), nt, 9, dtype)
            T, X = HostHeld(t), HostHeld(b)
            F.solve_lower_triangular_in_place(T.view, X.view)
            return finish({"x": X.view.copy(), "ref": np.linalg.solve(np.tril(t).astype(np.float64), b.astype(np.float64))}, [T, X])
        if family == "triangular_inverse":
            nt = 129
            t = (rnd(np.random.default_rng(6), nt, nt, dtype) / nt ** 0.5 + 2 * np.eye(nt, dtype=dtype)).astype(dtype)
            T, Out = HostHeld(t), HostHeld(np.full((nt, nt), -7.5, dtype=dtype))
            F.inverse_triangular_in_place(Out.view, T.view, upper=False, unit=False)
            return finish({"inv": Out.view.copy(), "ref": np.linalg.inv(np.tril(t).astype(np.float64))}, [T, Out])
        if family == "ldlt":
            A, R, Inv, X = (HostHeld(sentinel_upper(s_a)), HostHeld(np.full((n, n), -7.5, dtype=dtype)), HostHeld(np.full((n, n), -7.5, dtype=dtype)),
                            HostHeld(rnd(np.random.default_rng(7), n, 9, dtype)))
            rhs = X.view.copy()
            assert F.ldlt_factor_in_place(A.view) == 0
            F.ldlt_reconstruct(R.view, A.view)
            F.ldlt_inverse(Inv.view, A.view)
            F.ldlt_solve_in_place(A.view, X.view)
            return finish({"ld": A.view.copy(), "rec": R.view.copy(), "inv": Inv.view.copy(), "x": X.view.copy(), "ref": rhs}, [A, R, Inv, X])
        if family in ("tridiag", "hessenberg", "bidiag"):
            # the Householder coefficient matrices start from zeros, as in every test of these reductions: the upper triangles of their
            # diagonal blocks are defined, the cells below keep the caller's values
            from oracle import oracle as O

            nt, b_ = 67, 4
            x = np.random.default_rng(8).standard_normal((nt, nt))
            src = np.asarray(x + x.T if family == "tridiag" else x, dtype=dtype)
            if family == "bidiag":
                A, H, H2 = HostHeld(src), HostHeld(np.zeros((b_, nt), dtype=dtype)), HostHeld(np.zeros((b_, nt - 1), dtype=dtype))
                F.bidiag_in_place(A.view, H.view, H2.view)
                _, vo = place_host(src, "sub")
                ho, h2o = np.zeros((b_, nt), dtype=dtype, order="F"), np.zeros((b_, nt - 1), dtype=dtype, order="F")
                O.bidiag_in_place(vo, ho, h2o)
                return finish({"v": A.view.copy(), "h": H.view.copy(), "h2": H2.view.copy(), "a": src, "vo": vo.copy(), "ho": ho, "h2o": h2o}, [A, H, H2])
            A, H = HostHeld(src), HostHeld(np.zeros((b_, nt - 1), dtype=dtype))
            (F.tridiag_in_place if family == "tridiag" else F.hessenberg_in_place)(A.view, H.view)
            _, vo = place_host(src, "sub")
            ho = np.zeros((b_, nt - 1), dtype=dtype, order="F")
            (O.tridiag_in_place if family == "tridiag" else O.hessenberg_in_place)(vo, ho)
            return finish({"v": A.view.copy(), "h": H.view.copy(), "a": src, "vo": vo.copy(), "ho": ho}, [A, H])
        if family == "llt":
            A, R, Inv = HostHeld(sentinel_upper(s_a)), HostHeld(np.full((n, n), -7.5, dtype=dtype)), HostHeld(np.full((n, n), -7.5, dtype=dtype))
            assert F.llt_factor_in_place(A.view) == 0
            F.llt_reconstruct(R.view, A.view)
            F.llt_inverse(Inv.view, A.view)
            return finish({"l": A.view.copy(), "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, R, Inv])
        if family == "lu":
            A, R, Inv = HostHeld(a), HostHeld(nanm(n, n)), HostHeld(nanm(n, n))
            pf, pb, _ = F.partial_piv_lu_factor_in_place(A.view)
            F.partial_piv_lu_reconstruct(R.view, A.view, pf, pb)
            F.partial_piv_lu_inverse(Inv.view, A.view, pf, pb)
            return finish({"lu": A.view.copy(), "pf": pf, "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, R, Inv])
        if family == "full_piv_lu":
            A, R, Inv = HostHeld(a), HostHeld(nanm(n, n)), HostHeld(nanm(n, n))
            rf, rb, cf, cb, _ = F.full_piv_lu_factor_in_place(A.view)
            F.full_piv_lu_reconstruct(R.view, A.view, rf, rb, cf, cb)
            F.full_piv_lu_inverse(Inv.view, A.view, rf, rb, cf, cb)
            return finish({"lu": A.view.copy(), "rf": rf, "cf": cf, "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, R, Inv])
        if family in ("qr", "colpiv_qr"):
            bsz = F.qr_recommended_block_size(n, n, dtype)
            # (Q_coeff starts from zeros, as in every test of the family: the factorization defines the upper triangles of its diagonal
            # blocks only, the cells below them keep the caller's values)
            A, H, R, Inv = HostHeld(a), HostHeld(np.zeros((bsz, n), dtype=dtype)), HostHeld(nanm(n, n)), HostHeld(nanm(n, n))
            if family == "qr":
                assert F.qr_factor_in_place(A.view, H.view) == n
                F.qr_reconstruct(R.view, A.view, H.view)
                F.qr_inverse(Inv.view, A.view, H.view)
            else:
                cf, cb, _ = F.colpiv_qr_factor_in_place(A.view, H.view)
                F.colpiv_qr_reconstruct(R.view, A.view, H.view, cf, cb)
                F.colpiv_qr_inverse(Inv.view, A.view, H.view, cf, cb)
            return finish({"qr": A.view.copy(), "h": H.view.copy(), "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, H, R, Inv])
        if family == "svd":
            m = n + 9
            t = rnd(np.random.default_rng(3), m, n, dtype)
            A, U, V, S = HostHeld(t), HostHeld(nanm(m, n)), HostHeld(nanm(n, n)), HostHeld(nanm(n, 1))
            tag = F.svd(A.view, S.view[:, 0], U.view, V.view, svd_params(F, dtype, 4))
            return finish({"tag": tag, "a": t, "s": S.view[:, 0].copy(), "u": U.view.copy(), "v": V.view.copy()}, [A, U, V, S])
        if family == "evd":
            sy = np.asarray(a + a.T, dtype=dtype)
            A, U, S = HostHeld(sy), HostHeld(nanm(n, n)), HostHeld(nanm(n, 1))
            tag = F.self_adjoint_evd(A.view, S.view[:, 0], U.view, evd_params(F, dtype, 4))
            return finish({"tag": tag, "a": sy, "s": S.view[:, 0].copy(), "u": U.view.copy()}, [A, U, S])
        if family == "lblt":
            sy = np.asarray(a + a.T, dtype=dtype)
            A, R, Inv, Sub = HostHeld(sentinel_upper(sy)), HostHeld(np.full((n, n), -7.5, dtype=dtype)), HostHeld(nanm(n, n)), HostHeld(nanm(n, 1))
            _, pf, pb, _ = F.lblt_factor_in_place(A.view, subdiag=Sub.view[:, 0])
            F.lblt_reconstruct(R.view, A.view, Sub.view[:, 0], pf, pb)
            F.lblt_inverse(Inv.view, A.view, Sub.view[:, 0], pf, pb)
            return finish({"a": sy, "lb": A.view.copy(), "sub": Sub.view[:, 0].copy(), "pf": pf, "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, R, Inv, Sub])
        if family == "piv_llt":
            A, R, Inv = HostHeld(sentinel_upper(s_a)), HostHeld(np.full((n, n), -7.5, dtype=dtype)), HostHeld(np.full((n, n), -7.5, dtype=dtype))
            pf, pb, rank, _ = F.piv_llt_factor_in_place(A.view)
            F.piv_llt_reconstruct(R.view, A.view, pf, pb)
            F.piv_llt_inverse(Inv.view, A.view, pf, pb)
            return finish({"l": A.view.copy(), "pf": pf, "rank": rank, "rec": R.view.copy(), "inv": Inv.view.copy()}, [A, R, Inv])
        raise ValueError(family)

    def check(o):
        il, iu = np.tril_indices(n), np.triu_indices(n, 1)
        for k, v in o.items():
            if isinstance(v, np.ndarray) and v.dtype.kind == "f" and k not in ("ref", "a", "absprod", "vo", "ho", "h2o"):
                lower_only = (family in ("llt", "piv_llt") or (family == "lblt" and k in ("rec", "lb")) or (family == "ldlt" and k != "x")
                              or family == "triangular_inverse")
                if lower_only and v.ndim == 2:
                    assert (v[np.triu_indices(v.shape[0], 1)] == -7.5).all(), (k, "the strict upper triangle was written")
                    v = v[np.tril_indices(v.shape[0])]
                no_new_nan(v, None, f"{family} {k}")
        if family in ("matmul", "gemv"):  # test_matmul_vs_oracle bound(): 4 K eps |alpha| (|A| |B|) + 1e-300; the reference is the fp64 product
            kk = 1040 if family == "matmul" else 4100
            assert (np.abs(o["c"].astype(np.float64) - o["ref"]) <= 4 * kk * e * o["absprod"] + 1e-300).all()
        elif family == "trsm":  # test_trsm
            assert np.abs(o["x"] - o["ref"]).max() <= 64 * 129 * e * max(1.0, np.abs(o["ref"]).max())
        elif family == "triangular_inverse":  # test_triangular_inverse
            il9 = np.tril_indices(129)
            assert np.abs(o["inv"][il9] - o["ref"][il9]).max() <= 64 * 129 * e * max(1.0, np.abs(o["ref"]).max())
        elif family == "ldlt":  # test_ldlt_reconstruct_and_inverse; the solve as test_ldlt_solve_on_views bounds it in fp32 (test_llt_solve_vs_oracle)
            assert np.abs(o["rec"][il] - s_a[il]).max() <= 64 * n * e * np.abs(s_a).max()
            g = o["inv"].astype(np.float64)
            assert np.abs((np.tril(g) + np.tril(g, -1).T) @ s64 - np.eye(n)).max() <= 256 * n * e * np.linalg.cond(s64)
            xr = np.linalg.solve(s64, o["ref"].astype(np.float64))
            assert np.abs(o["x"].astype(np.float64) - xr).max() <= 64 * n * e * np.linalg.cond(s64) * max(1.0, np.abs(xr).max())
        elif family in ("tridiag", "hessenberg", "bidiag"):
            # test_tridiag_vs_oracle / test_hessenberg_vs_oracle / test_bidiag_vs_oracle: the condensed form normwise at 64 n eps ||A||_2
            # and the finite pattern of the block factors (the per-column reflector bounds run in test_tridiag / test_hessenberg / test_bidiag)
            nt = 67
            form = {"tridiag": tridiag_of, "hessenberg": hess_of, "bidiag": bidiag_of}[family]
            scale = np.linalg.norm(o["a"].astype(np.float64), 2)
            assert np.abs(form(o["v"]) - form(o["vo"])).max() <= 64 * nt * e * scale
            assert np.array_equal(np.isfinite(o["h"]), np.isfinite(o["ho"]))
            if family == "tridiag":
                fin = np.isfinite(o["ho"])
                assert np.abs(o["h"][fin] - o["ho"][fin]).max(initial=0.0) <= 64 * nt * e
            if family == "bidiag":
                assert np.array_equal(np.isfinite(o["h2"]), np.isfinite(o["h2o"]))
        elif family in ("llt", "piv_llt"):  # test_llt_reconstruct_and_inverse
            assert np.abs(o["rec"][il] - s_a[il]).max() <= 64 * n * e * np.abs(s_a).max()
            g = o["inv"].astype(np.float64)
            assert np.abs((np.tril(g) + np.tril(g, -1).T) @ s64 - np.eye(n)).max() <= 256 * n * e * np.linalg.cond(s64)
        elif family in ("lu", "full_piv_lu", "qr", "colpiv_qr"):  # test_lu_reconstruct_and_inverse and its siblings
            assert np.abs(o["rec"] - a).max() <= 64 * n * e * np.abs(a).max()
            assert np.abs(o["inv"].astype(np.float64) @ a64 - np.eye(n)).max() <= 256 * n * e * np.linalg.cond(a64)
        elif family == "svd":  # test_host_operands of tests/test_gpu_svd.py
            assert o["tag"] == F.SVD_OK
            svd_check(o["a"], o["s"], o["u"], o["v"])
        elif family == "evd":
            assert o["tag"] == F.EVD_OK
            evd_check(o["a"], o["s"], o["u"])
        elif family == "lblt":  # check_accuracy of tests/test_gpu_lblt.py
            sy = o["a"]
            assert np.abs(o["rec"][il].astype(np.float64) - sy[il]).max() <= 64 * n * e * np.abs(sy).max()
            inv, sy64 = o["inv"].astype(np.float64), sy.astype(np.float64)
            assert np.linalg.norm(sy64 @ inv - np.eye(n)) <= 64 * n * e * np.linalg.norm(sy64) * np.linalg.norm(inv)

    poisoned(F, fill, call, check, f"host operands {family} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ single-rank dist (dist.hip)
@pytest.mark.parametrize("what", ["lu", "llt"])
def test_dist_single_rank(oracle, fill, what):
    """test_dist_lu_device_backend_single_rank (700 x 500, nb = 96) / test_dist_llt_device_backend_single_rank (700, nb = 96)"""
    F = init_gpu()
    rng = np.random.default_rng(21)
    if what == "lu":
        m, n, nb = 700, 500, 96
        a = rnd(rng, m, n)
        ref = a.copy(order="F")
        perm, perm_inv, nt = oracle.lu_in_place(ref)
    else:
        m = n = 700
        nb = 96
        a = sentinel_upper(spd(rng, n, np.float64))
        ref = a.copy(order="F")
        assert oracle.llt_in_place(ref) == ("ok", 0)
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)

    def call():
        A = Held(a, "mat")
        da = A.view[:, :]
        if what == "lu":
            fwd, bwd, cnt = F.dist_partial_piv_lu(da, n, nb, 0, 1, lambda t, root: None)
            out = {"fwd": fwd, "bwd": bwd, "nt": cnt}
        else:
            out = {"count": F.dist_llt(da, n, nb, 0, 1, lambda t, root: None)}
        out["f"] = A.host()
        A.intact("dist " + what)
        return out

    def check(o):
        got = o["f"]
        no_new_nan(got, ref, "dist " + what)
        if what == "lu":
            assert np.array_equal(o["fwd"].astype(np.int64), perm) and np.array_equal(o["bwd"].astype(np.int64), perm_inv) and o["nt"] == nt
            assert np.abs(got - ref).max() <= 64 * max(m, n) * EPS[np.dtype(np.float64)] * max(1.0, np.abs(ref).max())
        else:
            assert o["count"] == 0 and (got[iu] == -7.5).all()
            assert np.abs(got[il] - ref[il]).max() <= 64 * n * EPS[np.dtype(np.float64)] * np.abs(ref[il]).max()

    poisoned(F, fill, call, check, f"dist {what} single rank")
