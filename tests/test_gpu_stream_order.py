"""Every family on a NON-BLOCKING caller stream (faer_hip_set_stream), both directions of the ordering contract.

The rest of the suite runs on the legacy null stream, which serialises against the library's blocking look-ahead streams by itself and so
hides a missing fork (an internal stream starts before the caller's pending work), a missing join (the caller's next operation starts
before an internal stream has finished), a stray null-stream operation inside a driver and a scratch buffer handed across streams too
early.  Here each case runs under gpu_util.ordered_call: the working buffers hold a STALE matrix of the same class (another seed, always
finite); on a torch side stream S -- delay (the library's own 4096^3 DGEMM, DELAY_PRODUCTS times), the copy of the good inputs into the
buffers (the producer), the public call, a copy of every output (the consumer), nothing in between on the host; then the host waits for
S alone.  A call that overtakes the producer factors the stale matrix; a call that returns with an internal stream still running
leaves unfinished outputs to the consumer.  The outcome is compared with the same call on the default stream, synchronised:
  * bit for bit where the suite already asserts that the path repeats itself bit for bit (the test is named at each case),
  * else at the bound of the entry point's dense test, named the same way;
  * permutations, ranks, counts, status codes and failing indices exactly.
test_stale_inputs_give_other_results shows on the CPU, once per family, that the stale seeds give results far beyond any of these bounds.

test_control_sees_a_lost_edge runs first: the producer on S, a matmul on a second stream with no event between them -- the caller's
own mistake -- must give the product of the STALE operands.  If it does not (a delay too short, both streams on one hardware queue),
every other test here would pass vacuously and the control says so.  What no test here can do: prove that an edge EXISTS between two
streams that happen to share a hardware queue -- the queue orders them by itself.

Entry points found (by reading) to return without a host synchronisation when their operands are device memory: matmul / gemm and the
triangular solves.  test_scratch_two_streams runs them back to back on two streams; every factorization ends with a host wait for the
caller's stream (its status word), after which only the first half of the protocol can fail by a missing fork and the second by a
missing join of an internal stream."""
import ctypes as C

import numpy as np
import pytest

import lblt_ref
import piv_llt_ref
from gpu_util import (DELAY_PRODUCTS, EPS, Routes, bits, delay, delay_operands, fa, init_gpu, on_stream, ordered_call, rnd, same_result, spd, to_dev)
from test_gpu_factor import LLT_STEP_KINDS
from test_gpu_self_adjoint_evd import sym
from test_gpu_views import quasi_definite, well_conditioned

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
GOOD, STALE = 1000, 2000  # seed offsets of the two sets of inputs


def close_result(expected, got, tol, what=""):
    """floating-point entries within tol[name] (absolute, entrywise) of `expected`, everything else exactly"""
    assert expected.keys() == got.keys(), (what, sorted(expected), sorted(got))
    for k, e in expected.items():
        g = got[k]
        if isinstance(e, np.ndarray) and e.dtype.kind == "f":
            assert np.isfinite(g).all(), (what, k)
            d = np.abs(g.astype(np.float64) - e.astype(np.float64)).max(initial=0.0)
            assert d <= tol[k], (what, k, d, tol[k])
        elif isinstance(e, np.ndarray):
            assert np.array_equal(e, g), (what, k)
        else:
            assert e == g, (what, k, e, g)


# ------------------------------------------------------------------------------------------ the control
def test_control_sees_a_lost_edge():
    """the producer on S, the consumer on S2, no event: the product of the stale operands (split-K shape of test_gemm_split_k,
    bitwise as test_split_k_lower_dst_is_bitwise_reproducible and the re-runs of test_gpu_scratch_poison.py assert)"""
    import torch

    F = init_gpu()
    m, n, k = 130, 70, 1030
    ops = {}
    for name, seed in (("good", GOOD), ("stale", STALE)):
        rng = np.random.default_rng(seed)
        ops[name] = (to_dev(rnd(rng, m, k)), to_dev(rnd(rng, k, n)))
    ref = {}
    for name, (a, b) in ops.items():
        c = to_dev(np.zeros((m, n)))
        F.matmul(c, F.ACCUM_REPLACE, a, b, 1.0)
        F.synchronize()
        ref[name] = c.cpu().numpy()
    assert np.abs(ref["good"] - ref["stale"]).max() > 1.0
    A, B = ops["stale"][0].clone(), ops["stale"][1].clone()
    cd, snap = to_dev(np.zeros((m, n))), to_dev(np.zeros((m, n)))
    delay_operands()
    S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with on_stream(S):
        delay(S)
        A.copy_(ops["good"][0], non_blocking=True)
        B.copy_(ops["good"][1], non_blocking=True)
    with on_stream(S2):
        F.matmul(cd, F.ACCUM_REPLACE, A, B, 1.0)
        snap.copy_(cd, non_blocking=True)
    S2.synchronize()
    got = snap.cpu().numpy()
    S.synchronize()
    what = "stale" if np.array_equal(bits(got), bits(ref["stale"])) else "good" if np.array_equal(bits(got), bits(ref["good"])) else "neither"
    print(f"control: the unordered consumer saw the {what} product after a delay of {DELAY_PRODUCTS} products")
    assert what == "stale", (f"the harness is blind in this process: a consumer on a second stream, not ordered after the producer, saw the "
                             f"{what} product -- the delay of {DELAY_PRODUCTS} products is too short or both streams share a hardware queue")


# ------------------------------------------------------------------------------------------ LLT look-ahead (potrf.hip)
def spd_dev(n, seed, dtype):
    import torch

    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.randn((n, n), dtype=dt, device="cuda", generator=g)
    return (b @ b.t() + n * torch.eye(n, dtype=dt, device="cuda")).t().clone()


def llt_fn(F):
    def fn(bufs):
        return {"count": F.llt_factor_in_place(bufs["a"]), "l": bufs["a"]}

    return fn


# n = 5197 with LLT_STEP_KINDS: every kind of step (follower, side-stream solve, split and merged updates) and the join at the end of
# LltLookahead::run; n = 3077 with a tail of 1024: look-ahead steps, then tail panels on the caller's stream.
# Bitwise: test_llt_lookahead_path ("same answer twice") runs these sizes and knobs.
@pytest.mark.parametrize("n,tail,knobs,dtype", [(5197, 0, LLT_STEP_KINDS, np.float64), (5197, 0, LLT_STEP_KINDS, np.float32), (3077, 1024, {}, np.float64)],
                         ids=["5197-step-kinds-f64", "5197-step-kinds-f32", "3077-tail-1024"])
def test_llt_lookahead(n, tail, knobs, dtype, monkeypatch):
    F = init_gpu()
    monkeypatch.setenv("FAER_HIP_LLT_LA_MIN", "2048")
    monkeypatch.setenv("FAER_HIP_LLT_TAIL", str(tail))
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    # the driver's own plan under these knobs (the planner test_cabi.py::test_driver_planning_logic_needs_no_gpu pins): four codes per step
    F.lib().faer_hip_debug_llt_steps.restype = C.c_size_t
    F.lib().faer_hip_debug_llt_plan.restype = C.c_size_t
    codes = (C.c_int * (4 * 16))()
    cnt = F.lib().faer_hip_debug_llt_steps(*(C.c_size_t(v) for v in (n, 2048, tail, int(knobs.get("FAER_HIP_LLT_SIDE_RMIN", 8192)),
                                                                      int(knobs.get("FAER_HIP_LLT_DPANEL_RMIN", 8192)))), codes, C.c_size_t(16))
    steps = [tuple(codes[4 * k:4 * k + 4]) for k in range(cnt)]
    assert cnt >= 1
    if knobs:  # every way a panel gets solved (side stream 0, follower 1, bulk 2), every update (last 0, merged 1, band 2, split 3), D_{k+1} on the panel stream (2)
        assert {s[0] for s in steps} == {0, 1, 2} and {s[1] for s in steps} == {0, 1, 2, 3} and 2 in {s[2] for s in steps}, steps
    else:  # look-ahead steps, then more than one 128-column tail panel on the caller's stream
        J = (C.c_size_t * 64)()
        nj = F.lib().faer_hip_debug_llt_plan(C.c_size_t(n), C.c_size_t(tail), C.c_size_t(1024), J, C.c_size_t(64))
        assert nj >= 2 and n - int(J[nj - 1]) > 128, list(J[:nj])
    good, stale = {"a": spd_dev(n, GOOD + n, dtype)}, {"a": spd_dev(n, STALE + n, dtype)}
    expected, got = ordered_call(llt_fn(F), good, stale)
    assert expected["count"] == 0
    same_result(expected, got, f"llt look-ahead {n}")


def test_llt_lookahead_failing_pivot(monkeypatch):
    """test_llt_lookahead_failure_index, side-stream-solve case: the bad pivot at 2000 of n = 5000; the stale matrix is positive
    definite, so a call that overtakes the producer reports success"""
    F = init_gpu()
    monkeypatch.setenv("FAER_HIP_LLT_LA_MIN", "2048")
    monkeypatch.setenv("FAER_HIP_LLT_TAIL", "0")
    for name, value in LLT_STEP_KINDS.items():
        monkeypatch.setenv(name, value)
    n, bad = 5000, 2000
    a = spd_dev(n, 5, np.float64)
    a[bad, bad] = -1.0

    def fn(bufs):
        try:
            return {"count": F.llt_factor_in_place(bufs["a"])}
        except F.LltError as e:
            return {"index": e.index}

    expected, got = ordered_call(fn, {"a": a}, {"a": spd_dev(n, STALE + n, np.float64)})
    assert expected == {"index": bad} and got == {"index": bad}, (expected, got)


# ------------------------------------------------------------------------------------------ partial-pivot LU (getrf.hip)
def lu_fn(F):
    def fn(bufs):
        perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(bufs["a"])
        return {"lu": bufs["a"], "perm": perm, "perm_inv": perm_inv, "nt": nt}

    return fn


def randn_dev(m, n, seed, dtype):
    import torch

    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    return torch.randn((n, m), dtype=dt, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)).t()


# all three phases of the look-ahead driver at n = 3072 (test_plu_lookahead_phases_and_transitions_at_small_n, plan (512, 1536, 2048));
# bitwise: that test ("the bitwise same answer twice") in fp64, test_plu_lookahead of test_gpu_scratch_poison.py in both precisions
@pytest.mark.parametrize("dtype", DTYPES)
def test_plu_lookahead(dtype):
    F = init_gpu()
    n = 3072
    good, stale = {"a": randn_dev(n, n, GOOD + n, dtype)}, {"a": randn_dev(n, n, STALE + n, dtype)}
    F.lib().faer_hip_debug_lu_plan(C.c_size_t(512), C.c_size_t(1536), C.c_size_t(2048))
    try:
        expected, got = ordered_call(lu_fn(F), good, stale)
    finally:
        F.lib().faer_hip_debug_lu_plan(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))
    assert sorted(expected["perm"].tolist()) == list(range(n))
    same_result(expected, got, f"lu look-ahead {n}")
    # the library has no counter of the LU driver's phases (the plan knob is all the existing tests have); at least the look-ahead driver
    # ran and not the tuned plan's flat / recursive one for this size: other rounding (fp64: with the same pivots)
    base = good["a"].clone()
    perm0, _, _ = F.partial_piv_lu_factor_in_place(base)
    F.synchronize()
    if dtype == np.float64:  # (test_plu_lookahead_phases_and_transitions_at_small_n; in fp32 the two drivers' rounding may pick other pivots)
        assert np.array_equal(perm0, expected["perm"])
    assert not np.array_equal(bits(base.cpu().numpy()), bits(expected["lu"])), "the plan knob did not change the driver"


# (600, 5): the cooperative leaf, bitwise as test_plu of test_gpu_scratch_poison.py re-runs it; (1000, 1000): the recursion, at the
# bound of test_plu_vs_oracle, 4 max(m, n) eps cond max(1, |ref|), with identical pivots
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(600, 5), (1000, 1000)])
def test_plu(m, n, dtype):
    F = init_gpu()
    good, stale = {"a": rnd(np.random.default_rng(GOOD + m), m, n, dtype)}, {"a": rnd(np.random.default_rng(STALE + m), m, n, dtype)}
    expected, got = ordered_call(lu_fn(F), good, stale)
    if m == 600:
        same_result(expected, got, f"lu {m}x{n}")
    else:
        size = min(m, n)
        kappa = np.linalg.cond(good["a"][expected["perm"].astype(np.int64)][:size, :size].astype(np.float64))
        tol = 4 * max(m, n) * EPS[np.dtype(dtype)] * kappa * max(1.0, np.abs(expected["lu"]).max())
        close_result(expected, got, {"lu": tol}, f"lu {m}x{n}")


# ------------------------------------------------------------------------------------------ QR (qr.hip, tsqr.hip)
# (20000, 64, 64) fp32 and (16500, 17, 1) fp64: the one-pass tall path (the smallest fp64 shape of test_qr_f64_tall_one_pass_vs_oracle);
# (33000, 384, 128): wide panels, the side stream; (512, 200): plain classic.  (2100, 320, 192) has 3 rows per column or more, so the
# whole matrix takes the one-pass path as well (its counter says so); (2100, 800, 192), under 3 rows per column, is the classic path whose
# recursion hands its panels of 1024 rows or more to the one-pass panel kernel.  No test asserts that this mixed path repeats itself bit for
# bit, so it is compared at the bounds of test_qr_classic_path_one_pass_panels_vs_oracle: 8 tol for the factor, 8 tol max(1, |T|) for
# Q_coeff, tol = 64 max(m, n) eps max(1, |A|) -- at most 0.7 here (fp32), where the diagonal of R is +-sqrt(m) = +-46 with signs that two
# independent matrices do not share.
# Bitwise: test_qr_is_bitwise_reproducible, test_qr_f64_tall_reproducible, and test_qr_classic / test_qr_one_pass /
# test_qr_one_pass_falls_back_per_panel of test_gpu_scratch_poison.py (equal re-runs of the classic, one-pass and mixed paths)
@pytest.mark.parametrize("m,n,bs,dtype,one_pass", [(20000, 64, 64, np.float32, True), (16500, 17, 1, np.float64, True), (33000, 384, 128, np.float32, True),
                                                  (33000, 384, 128, np.float64, True), (2100, 320, 192, np.float32, True), (2100, 800, 192, np.float32, None), (2100, 800, 192, np.float64, None), (512, 200, 32, np.float64, False),
                                                  (512, 200, 32, np.float32, False)])
def test_qr(m, n, bs, dtype, one_pass):
    F = init_gpu()
    size = min(m, n)
    F.lib().faer_hip_debug_qr_one_pass_columns.restype = C.c_long
    # (the cells of Q_coeff below the upper triangles of its diagonal blocks keep the caller's values: zeros, stale 0.5)
    good = {"a": rnd(np.random.default_rng(GOOD + m + n), m, n, dtype), "h": np.zeros((bs, size), dtype=dtype)}
    stale = {"a": rnd(np.random.default_rng(STALE + m + n), m, n, dtype), "h": np.full((bs, size), 0.5, dtype=dtype)}

    def fn(bufs):
        rank = F.qr_factor_in_place(bufs["a"], bufs["h"])
        return {"rank": rank, "cols": F.lib().faer_hip_debug_qr_one_pass_columns(), "qr": bufs["a"], "h": bufs["h"]}

    expected, got = ordered_call(fn, good, stale)
    assert expected["rank"] == size
    if one_pass is not None:
        assert expected["cols"] == (n if one_pass else -1), expected["cols"]
    else:
        # the classic driver (no column on the tall path) whose recursion hands panels to the one-pass panel kernel: with that switch
        # off (test_qr_classic_path_one_pass_panels_vs_oracle) the factors come out with other rounding
        assert expected["cols"] == -1, expected["cols"]
        F.lib().faer_hip_debug_qr_panels_one_pass(0)
        try:
            off = fn({k: to_dev(v) for k, v in good.items()})
            F.synchronize()
        finally:
            F.lib().faer_hip_debug_qr_panels_one_pass(1)
        assert off["rank"] == size and not np.array_equal(bits(off["qr"].cpu().numpy()), bits(expected["qr"])), "no panel took the one-pass kernel"
        tol = 64 * max(m, n) * EPS[np.dtype(dtype)] * max(1.0, np.abs(good["a"]).max())
        close_result(expected, got, {"qr": 8 * tol, "h": 8 * tol * max(1.0, np.abs(expected["h"]).max())}, f"qr {m}x{n} bs={bs}")
        return
    same_result(expected, got, f"qr {m}x{n} bs={bs}")


# ------------------------------------------------------------------------------------------ one small blocked shape per family
def _sym(seed, n, dtype):
    return sym(np.random.default_rng(seed), n, dtype)


def make(family, seed, dtype):
    """the inputs of one small case: {name: numpy array}; outputs that the call defines completely start from a seed-dependent fill"""
    rng = np.random.default_rng(seed)
    junk = lambda r, c: np.full((r, c), -7.5 if seed < STALE else -3.25, dtype=dtype)
    if family == "ldlt":
        return {"a": quasi_definite(rng, 640, dtype)[0]}
    if family == "lblt":
        n = 130
        return {"a": np.asarray(lblt_ref.random_symmetric(n, seed), dtype=dtype), "sub": junk(n, 1), "x": rnd(rng, n, 9, dtype), "rec": junk(n, n), "inv": junk(n, n)}
    if family == "piv_llt":
        n = 130
        return {"a": np.asarray(piv_llt_ref.spd(n, seed), dtype=dtype), "x": rnd(rng, n, 9, dtype), "rec": junk(n, n), "inv": junk(n, n)}
    if family == "fplu":
        return {"a": rnd(rng, 300, 300, dtype)}
    if family == "colpiv_qr":
        m, n = 200, 50
        return {"a": np.asarray(rng.standard_normal((m, n)) * np.logspace(0, -3, n)[None, :], dtype=dtype, order="F"), "h": junk(fa().qr_recommended_block_size(m, n, dtype), n)}
    if family == "tridiag":
        return {"a": _sym(seed, 300, dtype), "h": junk(16, 299)}
    if family == "hessenberg":
        return {"a": rnd(rng, 300, 300, dtype), "h": junk(16, 299)}
    if family == "bidiag":
        return {"a": rnd(rng, 300, 300, dtype), "hl": junk(16, 300), "hr": junk(16, 299)}
    if family == "evd":
        return {"a": _sym(seed, 257, dtype), "s": junk(257, 1), "u": junk(257, 257)}
    if family == "svd":
        return {"a": rnd(rng, 300, 200, dtype), "s": junk(200, 1), "u": junk(300, 200), "v": junk(200, 200)}
    if family == "trsm":
        n = 300
        return {"t": np.asarray(rnd(rng, n, n) + n * np.eye(n), dtype=dtype, order="F"), "x": rnd(rng, n, 64, dtype)}
    if family == "triangular_inverse":
        n = 300
        return {"t": (rnd(rng, n, n, dtype) / n ** 0.5 + 2 * np.eye(n, dtype=dtype)).astype(dtype), "inv": junk(n, n)}
    if family in ("matmul_split_k", "matmul_wide", "matmul_skinny"):
        m, n, k = {"matmul_split_k": (130, 70, 1030), "matmul_wide": (4096, 4096, 2048), "matmul_skinny": (7, 9, 1000)}[family]
        a = rnd(rng, m, k, dtype)
        if family == "matmul_skinny":  # (the reduce kernel of skinny.hip wants A with unit column stride: row major, as test_skinny_reduce uploads it)
            a = np.ascontiguousarray(a)
        return {"a": a, "b": rnd(rng, k, n, dtype), "c": rnd(rng, m, n, dtype)}
    if family == "llt_rebuild":
        n = 300
        return {"a": spd(rng, n, dtype), "x": rnd(rng, n, 9, dtype), "rec": junk(n, n), "inv": junk(n, n)}
    if family in ("lu_rebuild", "qr_rebuild"):
        n = 300
        d = {"a": well_conditioned(rng, n, dtype), "x": rnd(rng, n, 9, dtype), "rec": junk(n, n), "inv": junk(n, n)}
        if family == "qr_rebuild":
            d["h"] = junk(32, n)
        return d
    if family in ("dist_llt", "dist_lu"):
        return {"a": spd(rng, 512, np.float64) if family == "dist_llt" else rnd(rng, 512, 512)}
    raise ValueError(family)


def call(F, family, bufs):
    """the public calls of one small case on device tensors; returns {name: tensor or host value}"""
    b = bufs
    if family == "ldlt":
        return {"count": F.ldlt_factor_in_place(b["a"]), "ld": b["a"]}
    if family == "lblt":
        sub = b["sub"][:, 0]
        _, pf, pb, cnt = F.lblt_factor_in_place(b["a"], subdiag=sub)
        F.lblt_solve_in_place(b["a"], sub, pf, pb, b["x"])
        F.lblt_reconstruct(b["rec"], b["a"], sub, pf, pb)
        F.lblt_inverse(b["inv"], b["a"], sub, pf, pb)
        return {"lb": b["a"], "sub": b["sub"], "pf": pf, "pb": pb, "count": cnt, "x": b["x"], "rec": b["rec"], "inv": b["inv"]}
    if family == "piv_llt":
        pf, pb, rank, cnt = F.piv_llt_factor_in_place(b["a"])
        F.piv_llt_solve_in_place(b["a"], pf, pb, b["x"])
        F.piv_llt_reconstruct(b["rec"], b["a"], pf, pb)
        F.piv_llt_inverse(b["inv"], b["a"], pf, pb)
        return {"l": b["a"], "pf": pf, "pb": pb, "rank": rank, "count": cnt, "x": b["x"], "rec": b["rec"], "inv": b["inv"]}
    if family == "fplu":
        rf, rb, cf, cb, nt = F.full_piv_lu_factor_in_place(b["a"])
        return {"lu": b["a"], "rf": rf, "rb": rb, "cf": cf, "cb": cb, "nt": nt}
    if family == "colpiv_qr":
        cf, cb, nt = F.colpiv_qr_factor_in_place(b["a"], b["h"])
        return {"qr": b["a"], "h": b["h"], "cf": cf, "cb": cb, "nt": nt}
    if family in ("tridiag", "hessenberg"):
        (F.tridiag_in_place if family == "tridiag" else F.hessenberg_in_place)(b["a"], b["h"])
        return {"v": b["a"], "h": b["h"]}
    if family == "bidiag":
        F.bidiag_in_place(b["a"], b["hl"], b["hr"])
        return {"u": b["a"], "hl": b["hl"], "hr": b["hr"]}
    if family == "evd":
        return {"tag": F.self_adjoint_evd(b["a"], b["s"][:, 0], b["u"]), "s": b["s"], "u": b["u"]}
    if family == "svd":
        return {"tag": F.svd(b["a"], b["s"][:, 0], b["u"], b["v"]), "s": b["s"], "u": b["u"], "v": b["v"]}
    if family == "trsm":
        F.solve_lower_triangular_in_place(b["t"], b["x"])
        return {"x": b["x"]}
    if family == "triangular_inverse":
        F.inverse_triangular_in_place(b["inv"], b["t"], upper=False, unit=False)
        return {"inv": b["inv"]}
    if family.startswith("matmul"):
        F.matmul(b["c"], F.ACCUM_ADD, b["a"], b["b"], -0.5)
        return {"c": b["c"]}
    if family == "llt_rebuild":
        cnt = F.llt_factor_in_place(b["a"])
        F.llt_reconstruct(b["rec"], b["a"])
        F.llt_inverse(b["inv"], b["a"])
        F.llt_solve_in_place(b["a"], b["x"])
        return {"count": cnt, "l": b["a"], "x": b["x"], "rec": b["rec"], "inv": b["inv"]}
    if family == "lu_rebuild":
        pf, pb, nt = F.partial_piv_lu_factor_in_place(b["a"])
        F.partial_piv_lu_solve_in_place(b["a"], pf, pb, b["x"])
        F.partial_piv_lu_reconstruct(b["rec"], b["a"], pf, pb)
        F.partial_piv_lu_inverse(b["inv"], b["a"], pf, pb)
        return {"lu": b["a"], "pf": pf, "nt": nt, "x": b["x"], "rec": b["rec"], "inv": b["inv"]}
    if family == "qr_rebuild":
        rank = F.qr_factor_in_place(b["a"], b["h"])
        F.qr_solve_in_place(b["a"], b["h"], b["x"])
        F.qr_reconstruct(b["rec"], b["a"], b["h"])
        F.qr_inverse(b["inv"], b["a"], b["h"])
        return {"rank": rank, "qr": b["a"], "h": b["h"], "x": b["x"], "rec": b["rec"], "inv": b["inv"]}
    if family == "dist_llt":
        return {"count": F.dist_llt(b["a"], 512, 64, 0, 1, lambda t, root: None), "l": b["a"]}
    if family == "dist_lu":
        fwd, bwd, nt = F.dist_partial_piv_lu(b["a"], 512, 64, 0, 1, lambda t, root: None)
        return {"lu": b["a"], "fwd": fwd, "bwd": bwd, "nt": nt}
    raise ValueError(family)


# Bitwise, as the re-runs of tests/test_gpu_scratch_poison.py assert for each of these families (test_llt_ldlt, test_lblt, test_piv_llt,
# test_full_piv_lu, test_colpiv_qr, test_tridiag, test_hessenberg, test_bidiag, test_self_adjoint_evd, test_svd, test_trsm,
# test_triangular_inverse, test_gemm_split_k, test_skinny_reduce, test_cholesky_rebuild, test_pivoted_solves_and_rebuild,
# test_dist_single_rank), test_deterministic of test_gpu_self_adjoint_evd.py and test_gpu_svd.py, and the determinism section of
# test_gpu_level3_exact.py for the dense tiles.
SMALL = ["ldlt", "lblt", "piv_llt", "fplu", "colpiv_qr", "tridiag", "hessenberg", "bidiag", "evd", "svd", "trsm", "triangular_inverse",
         "matmul_split_k", "matmul_wide", "matmul_skinny", "llt_rebuild", "lu_rebuild", "qr_rebuild", "dist_llt", "dist_lu"]


# the dispatch routes a case is about: a planning change must not quietly turn it into a copy of the plain tile
ROUTES_OF = {"matmul_split_k": ("GemmSplitK",), "matmul_wide": ("GemmPipeWide",), "matmul_skinny": ("GemmSkinny",)}


# (the distributed drivers in fp64 only, like test_dist_lu_device_backend_single_rank)
@pytest.mark.parametrize("family,dtype", [(f, d) for f in SMALL for d in DTYPES if not (f.startswith("dist") and d == np.float32)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_small(family, dtype):
    F = init_gpu()
    good, stale = make(family, GOOD + len(family), dtype), make(family, STALE + len(family), dtype)
    expected, got = ordered_call(lambda bufs: call(F, family, bufs), good, stale, routes=ROUTES_OF.get(family, ()))
    assert expected.get("tag", 0) == 0, expected["tag"]
    same_result(expected, got, f"{family} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------ the stale seeds on the CPU
def cpu_result(oracle, family, d):
    """a plain fp64 result of the family's operation that the outputs above determine"""
    a = d.get("a", d.get("t")).astype(np.float64)
    if family in ("llt", "llt_rebuild", "dist_llt", "piv_llt"):
        return np.linalg.cholesky(a) if family != "piv_llt" else np.linalg.solve(a, d["x"].astype(np.float64))
    if family in ("lu", "lu_rebuild", "dist_lu", "fplu", "ldlt", "lblt"):
        if family in ("lu", "dist_lu"):
            ref = np.asfortranarray(a)
            oracle.lu_in_place(ref)
            return ref
        return np.linalg.solve(a, d["x"].astype(np.float64)) if "x" in d else np.linalg.inv(a)
    if family in ("qr", "qr_rebuild", "colpiv_qr"):
        return np.abs(np.linalg.qr(a)[1])
    if family in ("tridiag", "hessenberg", "bidiag"):  # (sorted spectra of two random matrices nearly coincide: the reduced matrix itself)
        from oracle import oracle as O

        v, n = np.asfortranarray(a), a.shape[0]
        if family == "bidiag":
            O.bidiag_in_place(v, np.zeros((16, n), order="F"), np.zeros((16, n - 1), order="F"))
        else:
            (O.tridiag_in_place if family == "tridiag" else O.hessenberg_in_place)(v, np.zeros((16, n - 1), order="F"))
        return v
    if family == "evd":
        return np.abs(np.linalg.eigh(a)[1])
    if family == "svd":
        return np.abs(np.linalg.svd(a, full_matrices=False)[0])
    if family == "trsm":
        return np.linalg.solve(np.tril(a), d["x"].astype(np.float64))
    if family == "triangular_inverse":
        return np.linalg.inv(np.tril(a))
    if family.startswith("matmul"):
        return d["c"] - 0.5 * (a @ d["b"].astype(np.float64))
    raise ValueError(family)


@pytest.mark.parametrize("family", SMALL + ["llt", "lu", "qr"])
def test_stale_inputs_give_other_results(oracle, family):
    """the seeds cannot collide: on the CPU the stale inputs give a result that differs from the good one by more than a tenth of its
    largest entry, where the comparisons above allow no difference at all; the one bounded case (test_plu, 1000 x 1000, whose bound
    grows with the condition number and in fp32 exceeds the entries) rests on the exact comparison of the pivots: the oracle's pivots
    of that case's own good and stale matrices differ"""
    if family in ("llt", "lu", "qr"):  # the big cases draw on the device; the same distributions at a small size
        rg, rs = np.random.default_rng(GOOD), np.random.default_rng(STALE)
        good, stale = ({"a": spd(rg, 300)}, {"a": spd(rs, 300)}) if family == "llt" else ({"a": rnd(rg, 300, 40)}, {"a": rnd(rs, 300, 40)})
    else:
        n = 512 if family == "matmul_wide" else None  # (the wide tile's operands cut to a corner: the same generator)
        good, stale = make(family, GOOD + len(family), np.float64), make(family, STALE + len(family), np.float64)
        if n:
            good, stale = ({k: v[:n, :n] for k, v in d.items()} for d in (good, stale))
    rg, rs = cpu_result(oracle, family, good), cpu_result(oracle, family, stale)
    assert np.abs(rg - rs).max() > 0.1 * np.abs(rg).max(), family
    if family == "lu":  # the inputs of test_plu's bounded case themselves, in both precisions
        for dtype in DTYPES:
            pg, ps = (oracle.lu_in_place(rnd(np.random.default_rng(seed + 1000), 1000, 1000, dtype))[0] for seed in (GOOD, STALE))
            assert not np.array_equal(pg, ps)


# ------------------------------------------------------------------------------------------ host operands
# Staging is synchronous (common.h Staged: the copies and the write-back wait on the caller's stream), so only the first half of the
# protocol applies: the call queues behind the delay on S and its results are in host memory when it returns.
# Bitwise: test_host_operands of test_gpu_scratch_poison.py re-runs both families.
@pytest.mark.parametrize("family", ["llt", "svd"])
def test_host_operands(family):
    import torch

    F = init_gpu()
    rng = np.random.default_rng(GOOD + 7)
    src = {"a": spd(rng, 300)} if family == "llt" else {"a": rnd(rng, 200, 120), "s": np.full((120, 1), -7.5), "u": np.full((200, 120), -7.5),
                                                       "v": np.full((120, 120), -7.5)}

    def fn(b):
        if family == "llt":
            return {"count": F.llt_factor_in_place(b["a"]), "l": b["a"]}
        return {"tag": F.svd(b["a"], b["s"][:, 0], b["u"], b["v"]), "s": b["s"], "u": b["u"], "v": b["v"]}

    expected = fn({k: v.copy(order="F") for k, v in src.items()})
    bufs = {k: v.copy(order="F") for k, v in src.items()}
    delay_operands()
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    with on_stream(S):
        delay(S)
        got = fn(bufs)
    S.synchronize()
    assert expected.get("count", 0) == 0 and expected.get("tag", 0) == 0
    same_result(expected, got, f"host operands {family}")


# ------------------------------------------------------------------------------------------ the scratch pool across streams
def _pool_cases(F):
    """small calls that take scratch: (name, inputs, fn); matmul (split-K: the partial sums) and trsm (its products' workspace slot)
    return without a host synchronisation"""
    out = []
    for i in range(2):
        rng = np.random.default_rng(50 + i)
        out.append((f"matmul{i}", {"a": rnd(rng, 130, 1030), "b": rnd(rng, 1030, 70), "c": rnd(rng, 130, 70)}, lambda b: call(F, "matmul_split_k", b)))
        out.append((f"trsm{i}", make("trsm", 60 + i, np.float64), lambda b: call(F, "trsm", b)))
    return out


def _reference(F, cases):
    import torch

    ref = {}
    for name, inputs, fn in cases:
        bufs = {k: to_dev(v) for k, v in inputs.items()}
        with Routes(F) as r:
            out = fn(bufs)
        if name.startswith("matmul"):
            r.assert_hit("GemmSplitK")
        ref[name] = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    return ref


@pytest.mark.parametrize("fill", [-1, 0xFF], ids=["plain", "poisoned"])
def test_scratch_two_streams(fill):
    """S1: delay, split-K matmul, trsm; at once S2: the same calls on other data; no host synchronisation until both are queued.
    Both results equal their synchronised references; with the pool poisoned (0xFF) a buffer handed across early shows as NaN"""
    import torch

    F = init_gpu()
    cases = _pool_cases(F)
    ref = _reference(F, cases)
    bufs = {name: {k: to_dev(v) for k, v in inputs.items()} for name, inputs, _ in cases}
    delay_operands()
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    F.debug_scratch_fill(fill)
    try:
        outs = {}
        with on_stream(S1):
            delay(S1)
            for name, _, fn in cases[:2]:
                outs[name] = fn(bufs[name])
        with on_stream(S2):
            for name, _, fn in cases[2:]:
                outs[name] = fn(bufs[name])
        S1.synchronize()
        S2.synchronize()
        fills = F.debug_scratch_fill_stats()[0]
    finally:
        F.debug_scratch_fill(-1)
    assert fills > 0 if fill >= 0 else fills == 0
    for name in outs:
        same_result(ref[name], {k: v.cpu().numpy() for k, v in outs[name].items()}, f"two streams {name}")


def test_scratch_alternating_streams():
    """S1 / S2 / the default stream in turn over 21 small calls of mixed families on a poisoned pool, all inputs uploaded beforehand
    and no host wait between the calls other than those the factorizations make themselves (on their own stream): matmul and trsm
    leave work in flight on the stream the next call moves away from.  Every result equals its reference and every call takes
    scratch (the fill counter grows).  The calls are short, so how much is still in flight at a hand-over is not controlled here:
    test_scratch_two_streams holds one stream busy for that."""
    import torch

    F = init_gpu()
    cases = _pool_cases(F)[:2]
    for fam in ("llt_rebuild", "lu_rebuild", "qr_rebuild", "colpiv_qr", "svd"):
        cases.append((fam, make(fam, GOOD + len(fam), np.float64), lambda b, fam=fam: call(F, fam, b)))
    ref = _reference(F, cases)
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    bufs = [{k: to_dev(v) for k, v in cases[i % len(cases)][1].items()} for i in range(21)]
    torch.cuda.synchronize()
    F.debug_scratch_fill(0xFF)
    try:
        seen, outs = 0, []
        for i in range(21):
            name, _, fn = cases[i % len(cases)]
            S = streams[i % 3]
            if S is None:
                outs.append(fn(bufs[i]))
            else:
                with on_stream(S):
                    outs.append(fn(bufs[i]))
            fills = F.debug_scratch_fill_stats()[0]
            assert fills > seen, (i, name, fills, seen)
            seen = fills
        streams[0].synchronize()
        streams[1].synchronize()
        F.synchronize()
    finally:
        F.debug_scratch_fill(-1)
    for i, out in enumerate(outs):
        name = cases[i % len(cases)][0]
        same_result(ref[name], {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, f"call {i} {name}")
