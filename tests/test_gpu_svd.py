"""-m gpu tests of libfaer_v0_23_svd_{f64,f32} (csrc/svd.hip: bidiagonalization, divide and conquer on the bidiagonal, two
block Householder back-transforms) against LAPACK's singular values and the defining properties A v = s u, A^T u = s v,
U^T U = I, V^T V = I.  Tolerances are multiples of N eps ||A||_2 (N eps for orthogonality) with N = max(m, n), computed
in fp64 on the host."""
import json
import os
import time

import numpy as np
import pytest

from gpu_util import EPS, init_gpu, to_dev, to_host

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
# Multiple of N eps ||A||_2 (values, residuals per column) and of N eps (orthogonality).  numpy's fp64 LAPACK SVD attains at
# most 2.09 in these units on the inputs below (the 2 x 2 case; every larger case stays at or below 1.2); the bound is twice
# that.  Measured on the GPU: 0.91 at worst over the random shapes, the request combinations, the deflation-heavy inputs and the
# fixture up to svd128; svd512 in fp32 with 4-entry leaves gave 9.36 (A v - s u) / 6.71 (A^T u - s v) before the root check of
# svd_secular_kernel, and 0.02 in a float32 transcription of the solver with it.  Every check prints
# its ratios and the running worst.
C_TOL = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bidiag_svd_cases.json")
WORST = {"v": 0.0}


def tdt(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def params(F, dtype, recursion_threshold=None, qr_ratio_threshold=None):
    p = getattr(F.lib(), "libfaer_v0_23_SvdParams_" + ("f64" if np.dtype(dtype) == np.float64 else "f32"))
    p.restype = F.SvdParams
    q = p()
    if recursion_threshold is not None:
        q.recursion_threshold = recursion_threshold
    if qr_ratio_threshold is not None:
        q.qr_ratio_threshold = qr_ratio_threshold
    return q


def vec_shape(rows, k, mode):
    return None if mode == "no" else (rows, k if mode == "thin" else rows)


def run(F, a, u="thin", v="thin", prm=None):
    """device call; u / v: "no", "thin" or "full".  Returns tag, s, u, v (numpy, None where not requested)."""
    import torch

    m, n = a.shape
    k = min(m, n)
    ad = to_dev(a)
    sd = torch.full((k,), -7.0, dtype=tdt(a.dtype), device="cuda")
    us, vs = vec_shape(m, k, u), vec_shape(n, k, v)
    ud = to_dev(np.full(us, -7.0, dtype=a.dtype)) if us else None
    vd = to_dev(np.full(vs, -7.0, dtype=a.dtype)) if vs else None
    tag = F.svd(ad, sd, ud, vd, prm)
    return tag, to_host(sd), (to_host(ud) if us else None), (to_host(vd) if vs else None)


def check(a, s, u, v, c=C_TOL, ref=None):
    m, n = a.shape
    N, k = max(m, n), min(m, n)
    eps = EPS[np.dtype(a.dtype)]
    a64 = a.astype(np.float64)
    if ref is None:
        ref = np.linalg.svd(a64, compute_uv=False)
    nrm = max(ref[0] if k else 0.0, np.finfo(np.float64).tiny)
    an = a64 / nrm
    s64 = s.astype(np.float64)
    assert np.all(np.isfinite(s64))
    assert np.all(s64 >= 0), "negative singular value"
    assert np.all(np.diff(s64) <= 0), "singular values not nonincreasing"
    worst = np.abs(s64 - ref).max() / nrm / (N * eps)
    msg = [f"values {worst:.2f}"]
    sn = s64 / nrm
    if u is not None and v is not None:
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        r1 = np.linalg.norm(an @ v64[:, :k] - u64[:, :k] * sn, axis=0).max() / (N * eps)
        r2 = np.linalg.norm(an.T @ u64[:, :k] - v64[:, :k] * sn, axis=0).max() / (N * eps)
        msg += [f"A v - s u {r1:.2f}", f"A^T u - s v {r2:.2f}"]
        worst = max(worst, r1, r2)
    for name, x in (("U", u), ("V", v)):
        if x is not None:
            x64 = x.astype(np.float64)
            o = np.abs(x64.T @ x64 - np.eye(x64.shape[1])).max() / (N * eps)
            msg.append(f"{name}^T {name} {o:.2f}")
            worst = max(worst, o)
    WORST["v"] = max(WORST["v"], worst)
    print(f"svd check {a.shape} {np.dtype(a.dtype).name}: " + ", ".join(msg) + f" (running worst {WORST['v']:.2f})")
    assert worst <= c, "; ".join(msg) + " [units of N eps ||A||, N eps]"


def rand(seed, m, n, dtype):
    return np.asarray(np.random.default_rng(seed).standard_normal((m, n)), dtype=dtype, order="F")


SHAPES = [(1, 1), (2, 2), (3, 2), (2, 3), (5, 5), (17, 16), (64, 64), (128, 128), (129, 127), (257, 256), (600, 600), (300, 200),
          (400, 200), (200, 400), (1000, 37), (37, 1000)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["thin", "full"])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_shapes(shape, mode, dtype):
    F = init_gpu()
    a = rand(1000 + shape[0] * 7 + shape[1], *shape, dtype)
    tag, s, u, v = run(F, a, mode, mode)
    assert tag == F.SVD_OK
    check(a, s, u, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_1025_by_1024(dtype):
    F = init_gpu()
    a = rand(5, 1025, 1024, dtype)
    tag, s, u, v = run(F, a)
    assert tag == F.SVD_OK
    check(a, s, u, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(300, 200), (200, 300)])
def test_all_request_combinations(shape, dtype):
    F = init_gpu()
    a = rand(11, *shape, dtype)
    N, eps = max(shape), EPS[np.dtype(dtype)]
    ref = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    base = None
    for mu in ("no", "thin", "full"):
        for mv in ("no", "thin", "full"):
            tag, s, u, v = run(F, a, mu, mv)
            assert tag == F.SVD_OK
            check(a, s, u, v, ref=ref)
            if base is None:
                base = s.astype(np.float64)
            assert np.abs(s.astype(np.float64) - base).max() <= C_TOL * N * eps * ref[0]


def test_unrequested_outputs_are_not_written():
    import torch

    F = init_gpu()
    a = rand(12, 60, 40, np.float64)
    ad = to_dev(a)
    sd = torch.zeros(40, dtype=torch.float64, device="cuda")
    guard = torch.full((64, 64), -7.0, dtype=torch.float64, device="cuda")
    # a view with no columns into the guard: nothing of it may change
    assert F.svd(ad, sd, guard[:60, :0], guard[:40, :0]) == F.SVD_OK
    assert bool((to_host_t(guard) == -7.0).all())


def to_host_t(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu()


def with_singular_values(seed, m, n, sv, dtype):
    rng = np.random.default_rng(seed)
    k = min(m, n)
    qu, _ = np.linalg.qr(rng.standard_normal((m, k)))
    qv, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return np.asarray((qu * np.asarray(sv, dtype=np.float64)) @ qv.T, dtype=dtype, order="F")


def deflation_cases(dtype):
    n = 300
    f64 = np.dtype(dtype) == np.float64
    rng = np.random.default_rng(3)
    cases = {
        "zero": np.zeros((n, n)),
        "identity": np.eye(n),
        "signed_diagonal": np.diag(rng.standard_normal(n)),
        "rank_one": np.outer(rng.standard_normal(n), rng.standard_normal(n)),
        "rank_10": with_singular_values(4, 400, n, [10.0 - i if i < 10 else 0.0 for i in range(n)], np.float64),
        "multiplicity_50": with_singular_values(5, n, n, np.repeat(np.arange(6, 0, -1.0), 50), np.float64),
        "cluster": with_singular_values(6, n, n, 1.0 + (1e-14 if f64 else 5e-7) * np.arange(n)[::-1], np.float64),
        "graded": with_singular_values(7, n, n, np.logspace(0, -15 if f64 else -6, n), np.float64),
        "ones_superdiagonal": np.eye(n) + np.diag(np.ones(n - 1), 1),
        "kahan_like": np.eye(n) + np.triu(-0.5 * np.ones((n, n)), 1),
    }
    if f64:
        cases["graded_1e-300"] = np.diag(np.logspace(0, -300, n))
        cases["scaled_1e150"] = rng.standard_normal((n, n)) * 1e150
        cases["scaled_1e-150"] = rng.standard_normal((n, n)) * 1e-150
    return {k: np.asarray(v, dtype=dtype, order="F") for k, v in cases.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
def test_deflation_heavy_inputs(dtype, rt):
    F = init_gpu()
    prm = params(F, dtype, rt)
    for name, a in deflation_cases(dtype).items():
        tag, s, u, v = run(F, a, prm=prm)
        assert tag == F.SVD_OK, name
        print(name, end=": ")
        check(a, s, u, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
def test_reference_bidiagonal_cases(dtype, rt):
    F = init_gpu()
    prm = params(F, dtype, rt)
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 6
    for name, c in cases.items():
        d, e = np.asarray(c["diag"]), np.asarray(c["offdiag"])
        a = np.asarray(np.diag(d) + np.diag(e[: len(d) - 1], 1), dtype=dtype, order="F")
        tag, s, u, v = run(F, a, prm=prm)
        assert tag == F.SVD_OK, name
        print(name, end=": ")
        check(a, s, u, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recursion_threshold_values(dtype):
    F = init_gpu()
    a = rand(21, 300, 300, dtype)
    N, eps = 300, EPS[np.dtype(dtype)]
    ref = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    out = {}
    for rt in (4, 16, 64, 128, 1000):
        tag, s, u, v = run(F, a, prm=params(F, dtype, rt))
        assert tag == F.SVD_OK
        check(a, s, u, v, ref=ref)
        out[rt] = (s, u, v)
    for rt in out:
        assert np.abs(out[rt][0].astype(np.float64) - out[4][0].astype(np.float64)).max() <= C_TOL * N * eps * ref[0]
    for rt in (128, 1000):  # clamped to the same leaf size as 64
        for x, y in zip(out[rt], out[64]):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_qr_ratio_threshold(dtype):
    F = init_gpu()
    a = rand(22, 400, 200, dtype)
    N, eps = 400, EPS[np.dtype(dtype)]
    ref = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    base = None
    for ratio in (1.0, 11.0 / 6.0, 4.0):
        for mode in ("thin", "full"):
            tag, s, u, v = run(F, a, mode, mode, prm=params(F, dtype, qr_ratio_threshold=ratio))
            assert tag == F.SVD_OK
            check(a, s, u, v, ref=ref)
            if base is None:
                base = s.astype(np.float64)
            assert np.abs(s.astype(np.float64) - base).max() <= C_TOL * N * eps * ref[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_operands(dtype):
    F = init_gpu()
    a = rand(23, 200, 150, dtype)
    tag, s, u, v = run(F, a)
    sh = np.full(150, -7.0, dtype=dtype)
    uh = np.full((200, 150), -7.0, dtype=dtype, order="F")
    vh = np.full((150, 150), -7.0, dtype=dtype, order="F")
    a0 = a.copy()
    assert F.svd(a, sh, uh, vh) == F.SVD_OK and tag == F.SVD_OK
    assert np.array_equal(a, a0)
    assert np.array_equal(sh, s) and np.array_equal(uh, u) and np.array_equal(vh, v)
    check(a, sh, uh, vh)


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_and_strided_s(dtype):
    import torch

    F = init_gpu()
    m, n = 90, 70
    a = rand(24, m, n, dtype)
    tag, s, u, v = run(F, a)
    assert tag == F.SVD_OK
    t = tdt(dtype)
    # A: row major inside a padded parent
    ap = torch.full((m + 6, n + 9), 3.0, dtype=t, device="cuda")
    ap[2 : 2 + m, 5 : 5 + n] = torch.from_numpy(a).cuda()
    ap0 = ap.clone()
    av = ap[2 : 2 + m, 5 : 5 + n]
    # U: offset view of a column-major parent, V: offset view of a row-major parent, S: stride 2
    up = torch.full((n + 8, m + 4), -7.0, dtype=t, device="cuda").t()  # (m + 4) x (n + 8), column major
    vp = torch.full((n + 5, n + 3), -7.0, dtype=t, device="cuda")
    sp = torch.full((2 * n,), -7.0, dtype=t, device="cuda")
    uv, vv, sv = up[3 : 3 + m, 1 : 1 + n], vp[4 : 4 + n, 2 : 2 + n], sp[::2]
    assert uv.stride(0) == 1 and vv.stride(1) == 1
    assert F.svd(av, sv, uv, vv) == F.SVD_OK
    F.synchronize()
    assert torch.equal(ap, ap0)
    assert np.array_equal(sv.cpu().numpy(), s) and np.array_equal(uv.cpu().numpy(), u) and np.array_equal(vv.cpu().numpy(), v)
    assert bool((sp[1::2] == -7.0).all())
    um = torch.ones_like(up, dtype=torch.bool)
    um[3 : 3 + m, 1 : 1 + n] = False
    vm = torch.ones_like(vp, dtype=torch.bool)
    vm[4 : 4 + n, 2 : 2 + n] = False
    assert bool((up[um] == -7.0).all()) and bool((vp[vm] == -7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic(dtype):
    F = init_gpu()
    a = rand(25, 260, 180, dtype)
    r1, r2 = run(F, a, "full", "full"), run(F, a, "full", "full")
    assert r1[0] == F.SVD_OK
    for x, y in zip(r1[1:], r2[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("shape", [(0, 0), (5, 0), (0, 5)])
def test_empty_shapes(shape):
    import torch

    F = init_gpu()
    m, n = shape
    ad = torch.zeros((m, n), dtype=torch.float64, device="cuda")
    sd = torch.zeros((0,), dtype=torch.float64, device="cuda")
    assert F.svd(ad, sd) == F.SVD_OK
    ud = torch.full((m, m), -7.0, dtype=torch.float64, device="cuda")
    vd = torch.full((n, n), -7.0, dtype=torch.float64, device="cuda")
    assert F.svd(ad, sd, ud if m else None, vd if n else None) == F.SVD_OK
    F.synchronize()
    # mod.rs:586-591: the left factor of the (transposed) problem is the identity, the other one is left alone
    if m >= n and m:
        assert torch.equal(ud.cpu(), torch.eye(m, dtype=torch.float64))
    if n > m:
        assert torch.equal(vd.cpu(), torch.eye(n, dtype=torch.float64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_is_no_convergence(dtype, bad):
    F = init_gpu()
    a = rand(26, 400, 300, dtype)
    a[17, 5] = bad
    t0 = time.time()
    for mode in ("thin", "no"):
        tag, _, _, _ = run(F, a, mode, mode)
        assert tag == F.SVD_NO_CONVERGENCE
    assert time.time() - t0 < 30


def test_size_2048_f64():
    F = init_gpu()
    a = rand(27, 2048, 2048, np.float64)
    tag, s, u, v = run(F, a)
    assert tag == F.SVD_OK
    check(a, s, u, v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
@pytest.mark.parametrize("n", [130, 300])
def test_scaled_to_the_ends_of_the_range(n, rt, dtype):
    """A * 2^k over the table of tests/range_cases.py (fp64 to 2^+-900, beyond the 1e+-150 of the deflation cases; fp32 to 2^-90 / 2^100,
    outside the safe range of plain fp32 sums of squares); n = 130: two leaves and one merge.  With vectors and values only; `check` is
    relative to ||A||."""
    import range_cases as rc

    F = init_gpu()
    a0 = rand(n + 7, n, n, dtype)
    for k in rc.K["svd"][np.dtype(dtype)]:
        a = rc.scaled(a0, k)
        assert rc.cap_ok(a)
        for mode in ("thin", "no"):
            tag, s, u, v = run(F, a, mode, mode, prm=params(F, dtype, recursion_threshold=rt))
            assert tag == F.SVD_OK, (k, mode)
            assert rc.cap_ok(s), (k, mode)
            try:  # `check` is relative to ||A||: it gets A and S times 2^-k, exactly, so that nothing it squares leaves the range of fp64
                check(a0, rc.unscale(s, k, 1), u, v)
            except AssertionError as e:
                raise AssertionError(f"2^{k}, vectors {mode}: {e}") from None
