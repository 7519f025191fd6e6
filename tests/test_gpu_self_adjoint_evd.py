"""-m gpu tests of libfaer_v0_23_self_adjoint_evd_{f64,f32} (csrc/evd.hip: tridiagonalization, divide and conquer on the
tridiagonal, block Householder back-transform) against LAPACK's eigvalsh and the defining properties A U = U diag(S),
U^T U = I.  Tolerances are multiples of n eps ||A||_2 (n eps for orthogonality), computed in fp64 on the host."""
import json
import os
import time

import numpy as np
import pytest

from gpu_util import EPS, init_gpu, to_dev, to_host

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
C_TOL = 2  # multiple of n eps ||A||_2 (values, residual per column) and of n eps (orthogonality); measured worst case 0.95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tridiag_evd_cases.json")


def tdt(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def sym(rng, n, dtype):
    a = rng.standard_normal((n, n))
    return np.asarray(a + a.T, dtype=dtype, order="F")


def with_spectrum(rng, lam, dtype):
    n = len(lam)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return np.asarray((a + a.T) / 2, dtype=dtype, order="F")


def tridiagonal(d, e, dtype=np.float64):
    t = np.diag(np.asarray(d, dtype=np.float64))
    if len(e):
        t += np.diag(np.asarray(e, dtype=np.float64), 1) + np.diag(np.asarray(e, dtype=np.float64), -1)
    return np.asarray(t, dtype=dtype, order="F")


def params(F, dtype, recursion_threshold):
    p = getattr(F.lib(), "libfaer_v0_23_SelfAdjointEvdParams_" + ("f64" if np.dtype(dtype) == np.float64 else "f32"))
    p.restype = F.SelfAdjointEvdParams
    q = p()
    q.recursion_threshold = recursion_threshold
    return q


def run(F, a, with_u=True, prm=None, order="F"):
    import torch

    n = a.shape[0]
    ad = to_dev(a, order)
    sd = torch.full((n,), -7.0, dtype=tdt(a.dtype), device="cuda")
    ud = to_dev(np.zeros((n, n), dtype=a.dtype)) if with_u else None
    tag = F.self_adjoint_evd(ad, sd, ud, prm)
    return tag, to_host(sd), (to_host(ud) if with_u else None)


def check(a, s, u, c=C_TOL):
    n = a.shape[0]
    eps = EPS[np.dtype(a.dtype)]
    a64 = a.astype(np.float64)
    nrm = max(np.linalg.norm(a64, 2), np.finfo(np.float64).tiny)
    s64 = s.astype(np.float64)
    assert np.all(np.isfinite(s64))
    assert np.all(np.diff(s64) >= 0), "eigenvalues not ascending"
    ref = np.linalg.eigvalsh(a64)
    err = np.abs(s64 - ref).max() / (n * eps * nrm)
    assert err <= c, f"eigenvalues: {err:.2f} n eps ||A||"
    if u is not None:
        u64 = u.astype(np.float64)
        res = np.linalg.norm(a64 @ u64 - u64 * s64, axis=0).max() / (n * eps * nrm)  # worst column: ||A u_j - s_j u_j||_2
        orth = np.abs(u64.T @ u64 - np.eye(n)).max() / (n * eps)
        assert res <= c, f"residual: {res:.2f} n eps ||A||"
        assert orth <= c, f"orthogonality: {orth:.2f} n eps"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 127, 128, 129, 255, 256, 257, 500, 1000, 2049])
def test_random_against_lapack(n, dtype):
    F = init_gpu()
    a = sym(np.random.default_rng(n), n, dtype)
    tag, s, u = run(F, a)
    assert tag == F.EVD_OK
    check(a, s, u)


def deflation_cases(dtype):
    rng = np.random.default_rng(5)
    n = 300
    v = rng.standard_normal(n)
    cases = {
        "zero": np.zeros((n, n)),
        "identity": np.eye(n),
        "diagonal": np.diag(rng.standard_normal(n)),
        "rank_one": np.outer(v, v),
        "multiplicity_50": with_spectrum(rng, np.repeat(np.arange(1.0, 7.0), 50), np.float64),
        "cluster_1e-14": with_spectrum(rng, 1.0 + np.arange(n) * 1e-14, np.float64),
        "wilkinson_21": tridiagonal(np.abs(np.arange(21) - 10.0), np.ones(20)),
        "glued_wilkinson": tridiagonal(np.tile(np.abs(np.arange(21) - 10.0), 12), np.concatenate([np.r_[np.ones(20), 1e-7]] * 12)[:-1]),
    }
    if np.dtype(dtype) == np.float64:
        cases["graded_1e-300"] = with_spectrum(rng, np.logspace(-300, 0, n), np.float64)
        cases["scaled_1e150"] = sym(rng, n, np.float64) * 1e150
        cases["scaled_1e-150"] = sym(rng, n, np.float64) * 1e-150
    return {k: np.asarray(x, dtype=dtype, order="F") for k, x in cases.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
def test_deflation_heavy_spectra(dtype, rt):
    F = init_gpu()
    for name, a in deflation_cases(dtype).items():
        tag, s, u = run(F, a, prm=params(F, dtype, rt))
        assert tag == F.EVD_OK, name
        try:
            check(a, s, u)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
def test_reference_tridiagonal_cases(dtype, rt):
    F = init_gpu()
    cases = json.load(open(GOLDEN))["cases"]
    for name, c in cases.items():
        a = tridiagonal(c["diag"], c["offdiag"], dtype)
        tag, s, u = run(F, a, prm=params(F, dtype, rt))
        assert tag == F.EVD_OK, name
        try:
            check(a, s, u)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 300, 1000])
def test_eigenvalues_only_match(n, dtype):
    F = init_gpu()
    a = sym(np.random.default_rng(n + 1), n, dtype)
    tag0, s0, _ = run(F, a, with_u=False)
    tag1, s1, _ = run(F, a)
    assert tag0 == tag1 == F.EVD_OK
    eps, nrm = EPS[np.dtype(dtype)], np.linalg.norm(a.astype(np.float64), 2)
    assert np.abs(s0.astype(np.float64) - s1).max() <= C_TOL * n * eps * nrm
    check(a, s0, None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recursion_threshold_values(dtype):
    F = init_gpu()
    n = 300
    a = sym(np.random.default_rng(3), n, dtype)
    eps, nrm = EPS[np.dtype(dtype)], np.linalg.norm(a.astype(np.float64), 2)
    ss = []
    for rt in (4, 16, 64, 128, 1000):
        tag, s, u = run(F, a, prm=params(F, dtype, rt))
        assert tag == F.EVD_OK
        check(a, s, u)
        ss.append(s.astype(np.float64))
    for s in ss[1:]:
        assert np.abs(s - ss[0]).max() <= C_TOL * n * eps * nrm
    # 128 and 1000 are clamped to leaves of 64 rows: the same launches as 64
    assert np.array_equal(ss[2], ss[3]) and np.array_equal(ss[2], ss[4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 64])
@pytest.mark.parametrize("with_u", [True, False])
def test_deterministic(dtype, rt, with_u):
    """n = 130: with 64-row leaves the smallest size that has two merge levels with unequal halves"""
    F = init_gpu()
    a = sym(np.random.default_rng(130), 130, dtype)
    (tag1, s1, u1), (tag2, s2, u2) = (run(F, a, with_u=with_u, prm=params(F, dtype, rt)) for _ in range(2))
    assert tag1 == tag2 == F.EVD_OK
    assert np.array_equal(s1, s2)
    if with_u:
        assert np.array_equal(u1, u2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_operands(dtype):
    F = init_gpu()
    n = 200
    a = sym(np.random.default_rng(9), n, dtype)
    s = np.zeros(n, dtype=dtype)
    u = np.zeros((n, n), dtype=dtype, order="F")
    assert F.self_adjoint_evd(a, s, u) == F.EVD_OK
    check(a, s, u)
    _, sd, ud = run(F, a)
    assert np.array_equal(s, sd) and np.array_equal(u, ud)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_major_views_and_strided_s(dtype):
    import torch

    F = init_gpu()
    n = 150
    a = sym(np.random.default_rng(11), n, dtype)
    td = tdt(dtype)
    big_a = torch.full((n + 5, n + 7), 123.0, dtype=td, device="cuda")
    big_a[2:2 + n, 3:3 + n] = torch.from_numpy(a).cuda()
    big_a_before = big_a.clone()
    av = big_a[2:2 + n, 3:3 + n]  # row-major submatrix view
    big_u = torch.full((n + 4, n + 3), 321.0, dtype=td, device="cuda").t()  # column-major parent
    uv = big_u[1:1 + n, 2:2 + n]
    s_buf = torch.full((2 * n,), 55.0, dtype=td, device="cuda")
    sv = s_buf[::2]
    assert F.self_adjoint_evd(av, sv, uv) == F.EVD_OK
    F.synchronize()
    assert torch.equal(big_a, big_a_before), "A or its parent was written"
    ub = big_u.cpu().numpy()
    mask = np.ones(ub.shape, bool)
    mask[1:1 + n, 2:2 + n] = False
    assert np.all(ub[mask] == 321.0), "U's gaps were written"
    assert torch.all(s_buf[1::2] == 55.0), "S's gaps were written"
    check(a, sv.cpu().numpy(), uv.cpu().numpy())
    # the same decomposition as a column-major dense call
    _, s2, u2 = run(F, a)
    assert np.array_equal(sv.cpu().numpy(), s2) and np.array_equal(uv.cpu().numpy(), u2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_upper_triangle_never_read_or_written(dtype):
    F = init_gpu()
    n = 260
    a = sym(np.random.default_rng(13), n, dtype)
    poisoned = a.copy(order="F")
    poisoned[np.triu_indices(n, 1)] = np.nan
    ad = to_dev(poisoned)
    before = to_host(ad).copy()
    import torch

    sd = torch.empty(n, dtype=tdt(dtype), device="cuda")
    ud = to_dev(np.zeros((n, n), dtype=dtype))
    assert F.self_adjoint_evd(ad, sd, ud) == F.EVD_OK
    after = to_host(ad)
    assert np.array_equal(np.isnan(before), np.isnan(after))
    assert np.array_equal(before[~np.isnan(before)], after[~np.isnan(after)]), "A was written"
    _, s, u = run(F, a)
    assert np.array_equal(to_host(sd), s) and np.array_equal(to_host(ud), u)


def test_empty_matrix():
    import torch

    F = init_gpu()
    a = torch.empty((0, 0), dtype=torch.float64, device="cuda")
    s = torch.empty((0,), dtype=torch.float64, device="cuda")
    u = torch.empty((0, 0), dtype=torch.float64, device="cuda")
    assert F.self_adjoint_evd(a, s, u) == F.EVD_OK
    assert F.self_adjoint_evd(a, s) == F.EVD_OK


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_input_is_no_convergence(dtype):
    F = init_gpu()
    n = 400
    for bad in (np.nan, np.inf):
        a = sym(np.random.default_rng(17), n, dtype)
        a[200, 100] = bad
        t0 = time.perf_counter()
        for with_u in (True, False):
            tag, _, _ = run(F, a, with_u=with_u)
            assert tag == F.EVD_NO_CONVERGENCE
        assert time.perf_counter() - t0 < 30.0


def test_size_4096_f64():
    F = init_gpu()
    n = 4096
    a = sym(np.random.default_rng(4096), n, np.float64)
    tag, s, u = run(F, a)
    assert tag == F.EVD_OK
    check(a, s, u)


@pytest.mark.parametrize("dtype,step", [(np.float64, 1e-15), (np.float32, 5e-7)])
@pytest.mark.parametrize("n", [600, 1000])
def test_runs_inside_gap_segments(n, dtype, step):
    """eigenvalues spaced about tol / 2 apart (tol = 8 eps max(|d|, |z|) of a merge, tridiag_evd.rs:404): a run of nearly
    equal d is measured from its first entry, so one gap-delimited stretch of the merged d holds many runs of 2-3 entries,
    each with its own reflector -- every one of them must reach the eigenvectors (residual), not only keep them orthonormal"""
    F = init_gpu()
    a = with_spectrum(np.random.default_rng(n), 1.0 + np.arange(n) * step, dtype)
    for rt in (4, 128):
        tag, s, u = run(F, a, prm=params(F, dtype, rt))
        assert tag == F.EVD_OK
        check(a, s, u)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rt", [4, 128])
@pytest.mark.parametrize("n", [130, 300])
def test_scaled_to_the_ends_of_the_range(n, rt, dtype):
    """A * 2^k over the table of tests/range_cases.py (fp64 to 2^+-900, beyond the 1e+-150 of the deflation cases; fp32 to 2^-90 / 2^100,
    where its dnc_scale_kernel / dnc_tscale_kernel rescaling and the fp32 norm accumulators leave the safe range for the first time);
    n = 130: two leaves and one merge.  With vectors and values only; `check` is relative to ||A||."""
    import range_cases as rc

    F = init_gpu()
    a0 = sym(np.random.default_rng(n + 7), n, dtype)
    for k in rc.K["evd"][np.dtype(dtype)]:
        a = rc.scaled(a0, k)
        assert rc.cap_ok(a)
        for with_u in (True, False):
            tag, s, u = run(F, a, with_u=with_u, prm=params(F, dtype, rt))
            assert tag == F.EVD_OK, (k, with_u)
            assert rc.cap_ok(s), (k, with_u)
            try:  # `check` is relative to ||A|| but squares residuals on the way (inf at 2^900, 0 at 2^-900): it gets A and S times 2^-k, exactly
                check(a0, rc.unscale(s, k, 1), u)
            except AssertionError as e:
                raise AssertionError(f"2^{k}, vectors {with_u}: {e}") from None
