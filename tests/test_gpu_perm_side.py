"""GPU tests of the permutation-carrying solve / reconstruct / inverse entry points of the older families -- partial-pivot LU,
full-pivot LU, column-pivot QR -- where the other files leave gaps:
  * both index types (u32 and u64) on factor, solve (both transposes), reconstruct and inverse: the two runs must return equal
    permutations and bit-identical floating-point results;
  * every mode of the column-pivot QR solve (lstsq -- square and tall --, solve, transpose);
  * host-resident (NumPy) right-hand sides and outputs through the column-pivot QR functions, dense and as a view with two
    non-unit strides (packed staging): the same bits as with a device operand, and not one element of the parent array outside
    the view touched.
Solves are judged against the oracle's own factors put through the oracle's triangular solves and reflectors
(tests/test_gpu_solve_oracle.py), reconstruct / inverse by definition against NumPy (tests/test_gpu_extras.py), with the bounds of
those files.  Every matrix is built so that the pivot search leaves the diagonal; a case that does not pivot fails."""
import numpy as np
import pytest

from gpu_util import EPS, bits, guard_intact, init_gpu, place_host, rnd, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu
ITYPES = [np.uint32, np.uint64]
DTYPES = [np.float64, np.float32]
NS = [1, 5, 65, 130]  # around the 64-wide factor leaves and the 128-wide TRSM leaf
QR_SHAPES = [(5, 5), (130, 130), (200, 65)]
KS = [1, 7]


def tol(n, dtype, c=64):  # tests/test_gpu_extras.py
    return c * max(n, 1) * EPS[np.dtype(dtype)]


def solve_tol(n, dtype, a, ref):  # tests/test_gpu_solve_oracle.py
    return 64 * n * EPS[np.dtype(dtype)] * np.linalg.cond(a.astype(np.float64)) * max(1.0, np.abs(ref).max())


def pivoting(rng, m, n, dtype, qr=False):
    """m x n (m >= n) with orthonormal columns, its rows and its columns scaled by shuffled geometric sequences from 1 down to
    1 / 16: the largest entry of a row, a column or the whole matrix is nowhere near the diagonal, the condition number is at
    most 256.  qr: the columns alone are scaled, from 1 down to 1 / 100 -- they stay orthogonal, so column pivoting takes them
    in the order of the scales, each decision with a margin of 3.6 % or more, the same in every precision and summation order"""
    q = np.linalg.qr(rng.standard_normal((m, n)))[0]
    if qr:
        return np.asarray(q * rng.permutation(np.logspace(0, -2, n))[None, :], dtype=dtype, order="F")
    r = rng.permutation(np.logspace(0, -np.log10(16.0), m))
    c = rng.permutation(np.logspace(0, -np.log10(16.0), n))
    return np.asarray(q * r[:, None] * c[None, :], dtype=dtype, order="F")


def moved(perm):
    """the forward permutation is not the identity (asked of every case with at least 5 rows / columns)"""
    return len(perm) < 5 or not np.array_equal(perm.astype(np.int64), np.arange(len(perm)))


def same(x, y):
    return np.array_equal(bits(np.ascontiguousarray(x)), bits(np.ascontiguousarray(y)))


def nan_out(m, n, dtype):
    return to_dev(np.full((m, n), np.nan, dtype=dtype, order="F"))


def both_index_types(run):
    """run(index type) -> (tuple of permutations / counts, tuple of float arrays): equal and bit-identical between u32 and u64;
    returns the u64 run"""
    (p32, f32), (p64, f64) = (run(it) for it in ITYPES)
    assert all(p.dtype == np.uint32 for p in p32 if isinstance(p, np.ndarray))
    assert all(p.dtype == np.uint64 for p in p64 if isinstance(p, np.ndarray))
    assert len(p32) == len(p64) and all(np.array_equal(x, y) for x, y in zip(p32, p64))
    assert len(f32) == len(f64) and all(same(x, y) for x, y in zip(f32, f64)), "u32 and u64 runs differ in their floating-point results"
    return p64, f64


def check_rebuild(a, rec, inv):
    m, n = a.shape
    assert np.abs(rec - a).max() <= tol(max(m, n), a.dtype) * np.abs(a).max()
    if inv is not None:
        a64 = a.astype(np.float64)
        assert np.abs(inv.astype(np.float64) @ a64 - np.eye(n)).max() <= tol(n, a.dtype, 256) * np.linalg.cond(a64)


# ------------------------------------------------------------------------------------------------ partial-pivot LU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_partial_piv_lu_index_types(oracle, n, k, dtype):
    F = init_gpu()
    rng = np.random.default_rng(100 * n + k)
    a, b = pivoting(rng, n, n, dtype), rnd(rng, n, k, dtype)
    lu = a.copy(order="F")
    perm, perm_inv, nt = oracle.lu_in_place(lu)

    def run(it):
        dlu = to_dev(a)
        pf, pb, cnt = F.partial_piv_lu_factor_in_place(dlu, index_dtype=it)
        x, xt = to_dev(b), to_dev(b)
        F.partial_piv_lu_solve_in_place(dlu, pf, pb, x)
        F.partial_piv_lu_solve_in_place(dlu, pf, pb, xt, transpose=True)
        rec, inv = nan_out(n, n, dtype), nan_out(n, n, dtype)
        F.partial_piv_lu_reconstruct(rec, dlu, pf, pb)
        F.partial_piv_lu_inverse(inv, dlu, pf, pb)
        return (pf, pb, cnt), tuple(to_host(t) for t in (dlu, x, xt, rec, inv))

    (pf, pb, cnt), (_, x, xt, rec, inv) = both_index_types(run)
    assert np.array_equal(pf, perm) and np.array_equal(pb, perm_inv) and cnt == nt and moved(pf)
    ref = np.asfortranarray(b[perm])  # A = P^T L U: x = U^-1 L^-1 (P b)
    oracle.trsm(lu, ref, unit=True)
    oracle.trsm(lu, ref, upper=True)
    assert np.abs(x.astype(np.float64) - ref).max() <= solve_tol(n, dtype, a, ref)
    ref = b.copy(order="F")  # A^T = U^T L^T P: x = P^T L^-T U^-T b
    oracle.trsm(lu.T, ref)
    oracle.trsm(lu.T, ref, upper=True, unit=True)
    ref = ref[perm_inv]
    assert np.abs(xt.astype(np.float64) - ref).max() <= solve_tol(n, dtype, a, ref)
    check_rebuild(a, rec, inv)


# ------------------------------------------------------------------------------------------------ full-pivot LU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_full_piv_lu_index_types(oracle, n, k, dtype):
    F = init_gpu()
    rng = np.random.default_rng(200 * n + k)
    a, b = pivoting(rng, n, n, dtype), rnd(rng, n, k, dtype)
    lu = a.copy(order="F")
    rp, rpi, cp, cpi, nt = oracle.full_piv_lu_in_place(lu)

    def run(it):
        dlu = to_dev(a)
        *perms, cnt = F.full_piv_lu_factor_in_place(dlu, index_dtype=it)
        x, xt = to_dev(b), to_dev(b)
        F.full_piv_lu_solve_in_place(dlu, *perms, x)
        F.full_piv_lu_solve_in_place(dlu, *perms, xt, transpose=True)
        rec, inv = nan_out(n, n, dtype), nan_out(n, n, dtype)
        F.full_piv_lu_reconstruct(rec, dlu, *perms)
        F.full_piv_lu_inverse(inv, dlu, *perms)
        return (*perms, cnt), tuple(to_host(t) for t in (dlu, x, xt, rec, inv))

    (rf, rb, cf, cb, cnt), (_, x, xt, rec, inv) = both_index_types(run)
    assert all(np.array_equal(g, w) for g, w in zip((rf, rb, cf, cb), (rp, rpi, cp, cpi))) and cnt == nt and moved(rf) and moved(cf)
    ref = np.asfortranarray(b[rp])  # P A Q = L U: x = Q U^-1 L^-1 (P b)
    oracle.trsm(lu, ref, unit=True)
    oracle.trsm(lu, ref, upper=True)
    ref = ref[cpi]
    assert np.abs(x.astype(np.float64) - ref).max() <= solve_tol(n, dtype, a, ref)
    ref = np.asfortranarray(b[cp])  # Q^T A^T P^T = U^T L^T: x = P^T L^-T U^-T (Q^T b)
    oracle.trsm(lu.T, ref)
    oracle.trsm(lu.T, ref, upper=True, unit=True)
    ref = ref[rpi]
    assert np.abs(xt.astype(np.float64) - ref).max() <= solve_tol(n, dtype, a, ref)
    check_rebuild(a, rec, inv)


# ------------------------------------------------------------------------------------------------ column-pivot QR
def colpiv_factor(F, a, it):
    m, n = a.shape
    dqr = to_dev(a)
    dh = to_dev(np.zeros((F.qr_recommended_block_size(m, n, a.dtype), min(m, n)), dtype=a.dtype, order="F"))
    cf, cb, cnt = F.colpiv_qr_factor_in_place(dqr, dh, index_dtype=it)
    return dqr, dh, cf, cb, cnt


def colpiv_modes(m, n):
    return ("lstsq", "solve", "transpose") if m == n else ("lstsq",)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m,n", QR_SHAPES)
def test_colpiv_qr_index_types_and_solve_modes(oracle, m, n, k, dtype):
    """(200, 65): the least-squares solution is the top 65 rows, and only they are permuted back"""
    F = init_gpu()
    rng = np.random.default_rng(300 * m + n + k)
    a, b = pivoting(rng, m, n, dtype, qr=True), rnd(rng, m, k, dtype)
    qr, h = a.copy(order="F"), np.zeros((oracle.qr_recommended_block_size(m, n, dtype), n), dtype=dtype, order="F")
    cp, cpi, nt = oracle.colpiv_qr_in_place(qr, h)
    modes = colpiv_modes(m, n)

    def run(it):
        dqr, dh, cf, cb, cnt = colpiv_factor(F, a, it)
        xs = [to_dev(b) for _ in modes]
        for mode, x in zip(modes, xs):
            F.colpiv_qr_solve_in_place(dqr, dh, cf, cb, x, mode=mode)
        outs = [nan_out(m, n, dtype)]
        F.colpiv_qr_reconstruct(outs[0], dqr, dh, cf, cb)
        if m == n:
            outs.append(nan_out(n, n, dtype))
            F.colpiv_qr_inverse(outs[1], dqr, dh, cf, cb)
        return (cf, cb, cnt), tuple(to_host(t) for t in [dqr, dh] + xs + outs)

    (cf, cb, cnt), (_, _, *res) = both_index_types(run)
    assert np.array_equal(cf, cp) and np.array_equal(cb, cpi) and cnt == nt and moved(cf)
    xs, outs = res[:len(modes)], res[len(modes):]
    ref = b.copy(order="F")  # A Q = H R: x = Q R^-1 (H^T b)[:n]
    oracle.apply_householder_sequence_left(qr, h, ref, True)
    top = np.asfortranarray(ref[:n])
    oracle.trsm(qr[:n, :n], top, upper=True)
    top = top[cpi]
    for mode, x in zip(modes, xs):
        if mode == "transpose":
            continue
        assert np.abs(x[:n].astype(np.float64) - top).max() <= solve_tol(max(m, n), dtype, a, top), mode
        if m > n:  # the rows below the solution keep the tail of H^T b: they are not part of the permutation
            assert np.abs(x[n:].astype(np.float64) - ref[n:]).max() <= solve_tol(m, dtype, a, ref)
    if m == n:
        assert same(xs[0], xs[1])  # lstsq and solve are the same computation on a square matrix
        ref = np.asfortranarray(b[cp])  # Q^T A^T = R^T H^T: x = H R^-T (Q^T b)
        oracle.trsm(qr.T, ref)
        oracle.apply_householder_sequence_left(qr, h, ref, False)
        assert np.abs(xs[2].astype(np.float64) - ref).max() <= solve_tol(n, dtype, a, ref)
    check_rebuild(a, outs[0], outs[1] if m == n else None)


def host_operand(x, placement):
    """(parent, view, box): `x` as a dense column-major NumPy array, or as every second row of a column-major parent with padded
    columns (layout "step2" of gpu_util: neither stride is 1, which takes the packed staging path)"""
    if placement == "dense":
        v = np.array(x, order="F")
        return v, v, None
    parent, v = place_host(x, placement)
    return parent, v, view_box(x.shape, placement, x.dtype)


@pytest.mark.parametrize("placement", ["dense", "step2"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m,n", QR_SHAPES)
def test_colpiv_qr_host_operands(m, n, k, dtype, placement):
    """the functions composed of the unpivoted QR routine and a permutation, with the operand they write in host memory: the bits
    of the device-operand run, nothing outside the view written"""
    F = init_gpu()
    rng = np.random.default_rng(400 * m + n + k)
    a, b = pivoting(rng, m, n, dtype, qr=True), rnd(rng, m, k, dtype)
    dqr, dh, cf, cb, _ = colpiv_factor(F, a, np.uint64)
    assert moved(cf)

    def both(x, call):
        """call(operand) with the values of `x` in a device operand and in the host one: returns the device result after comparing"""
        d = to_dev(x)
        call(d)
        parent, v, box = host_operand(x, placement)
        before = parent.copy()
        call(v)
        got = to_host(d)
        assert same(v, got), "host and device operands give different bits"
        if box is not None:
            guard_intact(parent, before, box, "host operand")
        return got

    for mode in colpiv_modes(m, n):
        x = both(b, lambda t: F.colpiv_qr_solve_in_place(dqr, dh, cf, cb, t, mode=mode))
        a64 = a.astype(np.float64)
        ref = np.linalg.lstsq(a64.T if mode == "transpose" else a64, b.astype(np.float64), rcond=None)[0]
        assert np.abs(x[:n] - ref).max() <= 64 * solve_tol(max(m, n), dtype, a, ref), mode  # the bound of tests/test_gpu_qr.py against lstsq
    rec = both(np.full((m, n), -7.5, dtype=dtype), lambda t: F.colpiv_qr_reconstruct(t, dqr, dh, cf, cb))
    inv = both(np.full((n, n), -7.5, dtype=dtype), lambda t: F.colpiv_qr_inverse(t, dqr, dh, cf, cb)) if m == n else None
    check_rebuild(a, rec, inv)
