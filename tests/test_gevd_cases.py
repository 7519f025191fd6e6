"""tests/gevd_cases.py alone (CPU): the recorded results of tests/golden/gevd_bounds.json and gevd_spectra.npz are current where scipy is installed, and
the reference solver passes both verdicts on every listed case and size, within the cap on pairs left out of the assignment."""
import importlib.util
import os

import numpy as np
import pytest

import gevd_cases as gc

spec = importlib.util.spec_from_file_location("make_gevd_bounds", os.path.join(os.path.dirname(gc.GOLDEN), "make_gevd_bounds.py"))
mk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mk)

CASES = [(kind, n, dtype) for dtype in gc.DTYPES for kind, n in mk.cases(dtype)]
IDS = [f"{k}-{n}-{np.dtype(d).name}" for k, n, d in CASES]


def test_golden_file_lists_exactly_the_cases():
    import json

    keys = set(json.load(open(gc.GOLDEN)))
    assert keys == {gc._key(k, n, d) for k, n, d in CASES}
    z = np.load(gc.GOLDEN_SPECTRA)
    total = sum(int(k.split("/")[1]) for k in keys)
    assert set(z.files) == {"alpha", "beta", "kappa"} and all(z[name].shape == (total,) for name in z.files)
    assert os.path.getsize(gc.GOLDEN) < (1 << 20) and os.path.getsize(gc.GOLDEN_SPECTRA) < (1 << 20)


@pytest.mark.parametrize("kind,n,dtype", CASES, ids=IDS)
def test_reference_passes_its_own_verdicts(kind, n, dtype):
    pytest.importorskip("scipy")
    a, b = gc.generate(kind, n, dtype)
    own = gc._compute(kind, n, dtype)
    ref = gc.reference(kind, n, dtype)
    gold = gc.reference(kind, n, dtype, prefer_golden=True)
    # the recorded results are current
    # the recorded results are current: the recorded spectrum is the live one to well within the radii (another build of LAPACK
    # rounds differently), the residuals and condition numbers agree in magnitude
    cur = dict(ref, radius=np.minimum(ref["radius"], 1.0) / 16)
    assert kind in gc.RESIDUAL_ONLY or gc.assign_pairs(gold["alpha"], gold["beta"], cur)[0]
    e = gc.eps_of(dtype)
    assert abs(gold["res_right"] - ref["res_right"]) <= n * e and abs(gold["res_left"] - ref["res_left"]) <= n * e
    if kind not in gc.RESIDUAL_ONLY:  # (beyond 1 / eps a condition number is noise; these kinds do not use them)
        assert np.allclose(np.sort(np.log2(gold["kappa"])), np.sort(np.log2(np.minimum(ref["kappa"], 3e38))), atol=1.0)
    br, bl = gc.bounds(kind, n, dtype)
    assert own["res_right"] <= br and own["res_left"] <= bl
    if kind in gc.RESIDUAL_ONLY:  # the residual verdict is the only one these kinds are checked under
        return
    # the reference in the dtype of the case against the fp64 reference: the assignment, and the cap on pairs left out
    ok, left_out = gc.assign_pairs(own["own_alpha"], own["own_beta"], ref)
    assert ok and left_out <= 0.1 * n, (left_out, n)
    if kind == "infinite_in_triangle":
        assert int((own["own_beta"] == 0).sum()) == len(gc.infinite_rows(n))
    if kind.startswith("singular_b"):
        k = gc.singular_count(kind, n)
        assert int((own["own_beta"] == 0).sum()) == k


def test_verdicts_reject_wrong_results():
    n, dtype = 17, np.float64
    a, b = gc.generate("random", n, dtype)
    own = gc._compute("random", n, dtype) if gc._sla is not None else None
    ref = gc.reference("random", n, dtype)
    al, be = ref["alpha"].copy(), ref["beta"].copy()
    assert gc.assign_pairs(al, be, ref)[0]
    assert gc.assign_pairs(al * 3.0, be * 3.0, ref)[0]  # a scaling of (alpha, beta) is the same eigenvalue
    al2 = al.copy()
    al2[0] = al2[1]
    be2 = be.copy()
    be2[0] = be2[1]
    assert not gc.assign_pairs(al2, be2, ref)[0]  # an eigenvalue reported twice, another one missing
    if own is not None:
        x = np.linalg.solve(a.astype(complex) * be[0] - b * al[0] + 1e-9 * np.eye(n), np.ones(n, complex))
        assert gc.pair_residuals(a, b, al[:1], be[:1], x[:, None]).max() < 1e-6
        assert gc.pair_residuals(a, b, al[:1], be[:1], np.ones((n, 1))).max() > 1e-3


def mk_sizes_range(dtype):
    """every size a range row runs at: tests/test_qz_host.py and tests/test_gpu_gevd.py"""
    W = mk.EDGES[np.dtype(dtype)]
    return gc.RANGE_HOST_SIZES + [W - 1, W + 1, 2 * W + 3]


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["f64", "f32"])
def test_range_table_is_representable(dtype):
    """the rows the issue names, unshrunk; every scaled input and expected output finite and normal, at every size"""
    rows = gc.range_rows(dtype)
    want = {np.dtype(np.float32): {(20, -20), (-20, 20), (40, -40), (-40, 40), (60, -60), (-60, 60), (60, 60), (-60, -60)},
            np.dtype(np.float64): {(100, -100), (-100, 100), (300, -300), (-300, 300), (480, -480), (-480, 480), (480, 480), (-480, -480)}}
    assert {(ka, kb) for _, ka, kb in rows} == want[np.dtype(dtype)] and len(rows) == 8
    for n in mk_sizes_range(dtype):
        for _, ka, kb in rows:
            assert gc.range_representable(n, dtype, ka, kb), (n, ka, kb)
    # and the assertion can fail: one binade short of the end of the format the smallest entries are subnormal
    k = -int(np.finfo(dtype).maxexp) + 3
    assert not gc.range_representable(17, dtype, k, k)


def packed(w, vr, vl, dtype):
    """a homogeneous complex result (conjugate pairs adjacent, +imag first) in the layout of the API: (alpha, alpha_im, beta, UR,
    UL); the second of a pair takes the conjugate of the first's (alpha, beta), whose beta LAPACK scales on its own"""
    n = w.shape[1]
    al, ai, be = (np.zeros(n, dtype=dtype) for _ in range(3))
    ur, ul = np.zeros((n, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    i = 0
    while i < n:
        al[i], ai[i], be[i] = w[0, i].real, w[0, i].imag, w[1, i].real
        assert w[1, i].imag == 0
        if ai[i] == 0:
            ur[:, i], ul[:, i] = vr[:, i].real, vl[:, i].real
            i += 1
        else:
            assert ai[i] > 0 and w[0, i + 1].imag < 0
            al[i + 1], ai[i + 1], be[i + 1] = al[i], -ai[i], be[i]
            for u, v in ((ur, vr), (ul, vl)):
                u[:, i], u[:, i + 1] = v[:, i].real, v[:, i].imag
            i += 2
    return al, ai, be, ur, ul


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["f64", "f32"])
def test_pair_residuals_at_the_ends_of_the_range(dtype):
    """the verdict on its own, on scaled A, B, alpha, beta: the unscaled values, nothing under- or overflows, a wrong column shows"""
    pytest.importorskip("scipy")
    n = 17
    a, b = gc.generate("random", n, dtype)
    al, be, vr, vl = gc._solve(a, b)
    base_r, base_l = gc.pair_residuals(a, b, al, be, vr), gc.pair_residuals(a, b, al, be, vl, "left")
    assert 0 < base_r.max() <= gc.bounds("random", n, dtype)[0]
    for ka, kb in [(500, -500), (-500, 500), (-500, -500), (500, 500)] + [(ka, kb) for _, ka, kb in gc.range_rows(dtype)]:
        sa, sb = np.ldexp(a.astype(np.float64), ka), np.ldexp(b.astype(np.float64), kb)
        sal, sbe = al * 2.0 ** ka, be * 2.0 ** kb
        with np.errstate(over="raise", invalid="raise"):
            r, l = gc.pair_residuals(sa, sb, sal, sbe, vr), gc.pair_residuals(sa, sb, sal, sbe, vl, "left")
        assert np.allclose(r, base_r, rtol=1e-6, atol=1e-20) and np.allclose(l, base_l, rtol=1e-6, atol=1e-20), (ka, kb)
        w = vr.copy()
        w[:, 3] = 1.0
        assert gc.pair_residuals(sa, sb, sal, sbe, w)[3] > 1e-3


RANGE = [(dtype, group, ka, kb) for dtype in gc.DTYPES for group, ka, kb in gc.range_rows(dtype)]


@pytest.mark.parametrize("dtype,group,ka,kb", RANGE, ids=[f"{np.dtype(d).name}-{g}-{ka}-{kb}" for d, g, ka, kb in RANGE])
def test_range_check_rejects_the_controls(dtype, group, ka, kb):
    """at every row: the reference solver's result on the unscaled pair, scaled as the row scales it, passes; with one wrong
    eigenvector column it fails, and with two entries of beta swapped it fails"""
    pytest.importorskip("scipy")
    n = 17
    a, b = gc.generate("random", n, dtype)
    w, vl, vr = gc._sla.eig(a, b, left=True, right=True, homogeneous_eigvals=True)
    assert w.dtype == np.result_type(dtype, np.complex64)
    al, ai, be, ur, ul = packed(w, vr, vl, dtype)
    al, ai, be = np.ldexp(al, ka), np.ldexp(ai, ka), np.ldexp(be, kb)
    gc.range_check(n, dtype, ka, kb, al, ai, be, ur, ul, verbose=False)
    real = np.nonzero(ai == 0)[0]
    assert real.size >= 2
    wrong = ur.copy()
    wrong[:, real[0]] = ur[:, real[1]]  # the eigenvector of another eigenvalue
    with pytest.raises(AssertionError):
        gc.range_check(n, dtype, ka, kb, al, ai, be, wrong, ul, verbose=False)
    wrong = ul.copy()
    wrong[:, real[0]] = ul[:, real[1]]
    with pytest.raises(AssertionError):
        gc.range_check(n, dtype, ka, kb, al, ai, be, ur, wrong, verbose=False)
    lam = al[real].astype(np.float64) / np.ldexp(be[real].astype(np.float64), ka - kb)
    i, j = real[lam.argmin()], real[lam.argmax()]
    assert be[i] != be[j]
    swapped = be.copy()
    swapped[i], swapped[j] = be[j], be[i]
    with pytest.raises(AssertionError):  # without vectors the assignment alone sees it
        gc.range_check(n, dtype, ka, kb, al, ai, swapped, verbose=False)
    with pytest.raises(AssertionError):
        gc.range_check(n, dtype, ka, kb, al, ai, swapped, ur, ul, verbose=False)


def test_vector_kinds_reach_the_guards():
    """in extended precision (gc.pair_guard_replay): graded_triangular_pair passes the threshold of the overflow guard at GUARD_N
    rows in either dtype, in fp64 at no smaller size, within one leaf; every divisor of jordan_pair is the pivot floor; the vector
    of an infinite eigenvalue (acoef == 0) meets no floor but the one of its own zeros"""
    assert gc.GUARD_N <= min(mk.EDGES.values())
    for dtype in gc.DTYPES:
        big = gc.guard_threshold(dtype)
        assert big == pytest.approx({np.float64: 6.7e153, np.float32: 9.2e18}[dtype], rel=1e-2)
        top, fired, floored, _ = gc.pair_guard_replay(*gc.generate("graded_triangular_pair", gc.GUARD_N, dtype), dtype)
        print(f"graded_triangular_pair n={gc.GUARD_N} {np.dtype(dtype).name}: largest unscaled component {float(top):.3e}, threshold {big:.3e}, fires {fired} times")
        assert top > big and fired > 0 and (floored == 0 or dtype == np.float32)  # (in fp32 the nearest ratios also meet the pivot floor)
        a, b = gc.generate("graded_triangular_pair", gc.GUARD_N, dtype)
        lam = np.diag(a).astype(np.float64) / np.diag(b)
        assert (np.diff(lam) >= 0.5e-3).all()  # distinct in the dtype, 1e-3 apart
        for n in (15, 35):
            top, fired, floored, divisors = gc.pair_guard_replay(*gc.generate("jordan_pair", n, dtype), dtype)
            assert floored == divisors == n * (n - 1) // 2 and fired > 0
        for n in (35, gc.GUARD_N):
            a, b = gc.generate("infinite_in_triangle", n, dtype)
            assert np.array_equal(np.nonzero(np.diag(b) == 0)[0], gc.infinite_rows(n)) and len(gc.infinite_rows(n)) == 3
            top, fired, floored, divisors = gc.pair_guard_replay(a, b, dtype)
            assert fired == 0 and floored == 3  # beta == 0 three times: M = -alpha B has the other two zeros of diag(B) on its diagonal
            assert top < big
    top, fired, _, _ = gc.pair_guard_replay(*gc.generate("graded_triangular_pair", gc.GUARD_N - 1, np.float64), np.float64)
    assert fired == 0 and top < gc.guard_threshold(np.float64)


def test_vector_kind_generators():
    for dtype in gc.DTYPES:
        for kind in gc.TRIANGLE_KINDS:
            for n in (15, gc.GUARD_N):
                a, b = gc.generate(kind, n, dtype)
                assert a.dtype == b.dtype == np.dtype(dtype) and (np.tril(a, -1) == 0).all() and (np.tril(b, -1) == 0).all() and (np.diag(b) >= 0).all()
                ra, rb = gc.generate("rotated_" + kind, n, dtype)
                assert np.count_nonzero(np.tril(ra, -1)) > n and abs(np.linalg.norm(ra.astype(np.float64)) / np.linalg.norm(a.astype(np.float64)) - 1) < 1e-5
                assert abs(np.linalg.norm(rb.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)) - 1) < 1e-5
