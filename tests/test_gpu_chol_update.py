"""Cholesky rank-r update / downdate and row-and-column deletion on the GPU (csrc/chol_update.hip) against the numpy restatement of
the reference (tests/chol_update_ref.py).  All sizes are in terms of (NB, RC) read from the library.

Bounds.  Residual: the new factor reproduces the modified matrix to 64 n eps max|A| -- the `tol` of test_gpu_piv_llt.py; max|A| is
that of the larger matrix of the pair, the factored one for a downdate (chol_update_ref.case_update says why and what the
restatement reaches).  Parity ring: |L_gpu - L_ref| / max|L_ref| over the lower triangle is at most 4 n eps.  The rule of
test_schur_host.py allows 4 x what the host build of the same bodies measures against the restatement, or 4 n eps, whichever
is larger; on exactly the inputs of this file the host build measures at most 0.042 n eps in fp64 (LLT downdate, n = 64, r = 65) and
below 0.001 n eps in fp32, so 4 n eps it is.  Measured on the device: at most 0.042 n eps (fp64), 0.000 (fp32); deletion 0.003 n eps.
The figures of every case are printed."""
import ctypes as C

import numpy as np
import pytest

import chol_update_ref as ref
from gpu_util import EPS, LAYOUTS, bits, fa, guard_intact, init_gpu, ordered_call, place, place_host, same_result, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]


def shape(dtype):
    return fa().chol_update_shape(dtype)


def sizes(dtype):
    nb, rc = shape(dtype)
    return [1, 2, 3, nb - 1, nb, nb + 1, 2 * nb + 1, 200], sorted({1, rc - 1, rc, rc + 1, 2 * rc + 1} - {0})


def dvec(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def product(ldlt):
    return ref.ldlt_product if ldlt else ref.llt_product


def gpu_update(F, f, w, alpha, ldlt):
    dl, dw, da = to_dev(f), to_dev(w), dvec(alpha)
    if ldlt:
        F.ldlt_rank_r_update_clobber(dl, dw, da)
    else:
        assert F.llt_rank_r_update_clobber(dl, dw, da) is None
    return to_host(dl)


_REF = {}


def ref_update(n, r, dtype, ldlt, downdate):
    """the case and the restatement's result, computed once per case"""
    key = (n, r, np.dtype(dtype).name, ldlt, downdate)
    if key not in _REF:
        f, w, alpha, target, amax = ref.case_update(n, r, dtype, ldlt, downdate)
        g = f.copy(order="F")
        (ref.ldlt_rank_r_update_clobber if ldlt else ref.llt_rank_r_update_clobber)(g, w.copy(order="F"), alpha.copy())
        _REF[key] = (f, w, alpha, target, amax, g)
    return _REF[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("downdate", [False, True])
@pytest.mark.parametrize("ldlt", [False, True])
def test_residual_counters_and_parity(ldlt, downdate, dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    ns, rs = sizes(dtype)
    eps = EPS[np.dtype(dtype)]
    worst_res = worst_par = 0.0
    for n in ns:
        for r in rs:
            f, w, alpha, target, amax, want = ref_update(n, r, dtype, ldlt, downdate)
            got = gpu_update(F, f, w, alpha, ldlt)
            last = F.debug_chol_update_last()
            blocks, chunks = -(-n // nb), -(-r // rc)
            assert last == {"blocks": blocks, "tail_launches": (blocks - 1) * chunks, "chunks": chunks, "loop_syncs": 0}, (n, r, last)
            assert np.array_equal(bits(np.triu(got, 1)), bits(np.triu(f, 1)))
            err = np.abs(product(ldlt)(got) - target).max()
            res = err / (n * eps * amax)
            par = np.abs(np.tril(got).astype(np.float64) - np.tril(want)).max() / (n * eps * np.abs(np.tril(want)).max())
            worst_res, worst_par = max(worst_res, res), max(worst_par, par)
            assert res <= 64, (n, r, res)
            assert par <= 4, (n, r, par)  # host build of the same bodies on these inputs: 0.042 n eps; the device: 0.042 n eps
    print(f"ldlt={ldlt} downdate={downdate} {np.dtype(dtype).name}: worst residual {worst_res:.2f} n eps max|A|, worst distance to the restatement {worst_par:.3f} n eps")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bitwise_equal(dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    for ldlt in (False, True):
        f, w, alpha, _, _, _ = ref_update(2 * nb + 1, 2 * rc + 1, dtype, ldlt, False)
        a, b = gpu_update(F, f, w, alpha, ldlt), gpu_update(F, f, w, alpha, ldlt)
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(dtype):
    F = init_gpu()
    one = np.ones(3, dtype=dtype)
    got = gpu_update(F, np.diag(np.array([3, 5, 8], dtype=dtype)), np.diag(np.array([4, 12, 15], dtype=dtype)), one, False)
    assert np.array_equal(bits(got), bits(np.diag(np.array([5, 13, 17], dtype=dtype))))
    # two columns of W on the same row: 3 -> 5 -> 13
    got = gpu_update(F, np.diag(np.array([3, 7], dtype=dtype)), np.array([[4, 12], [0, 0]], dtype=dtype), one[:2], False)
    assert np.array_equal(bits(got), bits(np.diag(np.array([13, 7], dtype=dtype))))
    # d == 0 && nd == 0: one nonzero per column of W, the result stays diagonal; then the single column (1, 0, 1)
    got = gpu_update(F, np.diag(np.array([1, 0, 1], dtype=dtype)), np.diag(np.array([1, 0, 1], dtype=dtype)), one, True)
    assert np.array_equal(bits(got), bits(np.diag(np.array([2, 0, 2], dtype=dtype))))
    got = gpu_update(F, np.diag(np.array([1, 0, 1], dtype=dtype)), np.array([[1], [0], [1]], dtype=dtype), one[:1], True)
    assert np.array_equal(bits(got), bits(np.array([[2, 0, 0], [0, 0, 0], [0.5, 0, 1.5]], dtype=dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_status(dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    n = 2 * nb + 1
    cases = [(j, 1, 0) for j in (5, nb + 1, n - 1)] + [(nb + 1, rc + 2, rc + 1)]
    for j, r, k in cases:
        l = np.asfortranarray(2 * np.eye(n, dtype=dtype))
        w = np.zeros((n, r), dtype=dtype, order="F")
        w[j, k] = 3
        alpha = -np.ones(r, dtype=dtype)
        dl, dw, da = to_dev(l), to_dev(w), dvec(alpha)
        with pytest.raises(F.LltError) as e:
            F.llt_rank_r_update_clobber(dl, dw, da)
        with pytest.raises(ref.NonPositivePivot) as want:
            ref.llt_rank_r_update_clobber(l, w, alpha)
        assert e.value.index == want.value.index == j
        assert F.llt_rank_r_update_clobber(to_dev(l), to_dev(w), dvec(alpha), raise_on_error=False) == j
        # a good call straight after the failed one
        f, w2, a2, _, _, g = ref_update(nb + 1, 1, dtype, False, False)
        got = gpu_update(F, f, w2, a2, False)
        assert np.abs(np.tril(got) - np.tril(g)).max() <= 4 * (nb + 1) * EPS[np.dtype(dtype)] * np.abs(g).max()
    # a later chunk fails at a smaller column of the same block than an earlier one
    l = np.asfortranarray(2 * np.eye(n, dtype=dtype))
    w = np.zeros((n, rc + 1), dtype=dtype, order="F")
    w[9, 0] = 3
    w[4, rc] = 3
    assert F.llt_rank_r_update_clobber(to_dev(l), to_dev(w), dvec(-np.ones(rc + 1, dtype=dtype)), raise_on_error=False) == 4
    # a NaN passes the pivot test: Ok, NaN in L
    f, w, alpha, _, _, _ = ref_update(n, 2, dtype, False, False)
    w = w.copy(order="F")
    w[nb, 0] = np.nan
    got = gpu_update(F, f, w, alpha, False)
    assert np.isnan(got[nb, nb]) and np.isnan(got[n - 1, nb]) and np.isfinite(np.tril(got)[:nb, :nb]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("it", [np.uint32, np.uint64])
def test_deletion(it, dtype):
    F = init_gpu()
    nb, _ = shape(dtype)
    eps = EPS[np.dtype(dtype)]
    worst = worst_par = 0.0
    for n in (3, nb + 1, 2 * nb + 1, 200):
        for name, idx in ref.index_sets(n):
            ld, a = ref.case_delete(n, dtype)
            dl = to_dev(ld)
            out = F.ldlt_delete_rows_and_cols_clobber(dl, idx, index_dtype=it)
            assert out.dtype == it and list(out) == sorted(idx)
            got = to_host(dl)
            assert np.array_equal(bits(np.triu(got, 1)), bits(np.triu(ld, 1)))
            last = F.debug_chol_update_last()
            keep = np.setdiff1d(np.arange(n), idx)
            m = len(keep)
            assert last["loop_syncs"] == 0 and last["blocks"] == -(-(m - min(idx)) // nb), (name, last)
            if m == 0:
                continue
            res = np.abs(ref.ldlt_product(got[:m, :m]) - a[np.ix_(keep, keep)]).max() / (n * eps * np.abs(a).max())
            ref.ldlt_delete_rows_and_cols_clobber(ld, idx)
            par = np.abs(np.tril(got[:m, :m]).astype(np.float64) - np.tril(ld[:m, :m])).max() / (n * eps * np.abs(np.tril(ld[:m, :m])).max())
            worst, worst_par = max(worst, res), max(worst_par, par)
            assert res <= 64, (n, name, res)
            assert par <= 4, (n, name, par)
    print(f"deletion {np.dtype(dtype).name} {np.dtype(it).name}: worst residual {worst:.2f} n eps max|A|, worst distance to the restatement {worst_par:.3f} n eps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_views(layout, dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    n, r = nb + 3, rc + 1
    for ldlt in (False, True):
        f, w, alpha, _, _, want = ref_update(n, r, dtype, ldlt, True)
        f = np.tril(f) + np.triu(np.full((n, n), np.nan, dtype=dtype), 1)  # the strict upper triangle is never read
        lp, lv = place(f, layout)
        wp, wv = place(w, layout)
        lp0, wp0 = lp.clone(), wp.clone()
        (F.ldlt_rank_r_update_clobber if ldlt else F.llt_rank_r_update_clobber)(lv, wv, dvec(alpha))
        F.synchronize()
        guard_intact(lp, lp0, view_box(f.shape, layout, dtype), "L")
        guard_intact(wp, wp0, view_box(w.shape, layout, dtype), "W")
        got = lv.cpu().numpy()
        assert np.array_equal(bits(np.triu(got, 1)), bits(np.triu(f, 1)))
        assert np.abs(np.tril(got) - np.tril(want)).max() <= 4 * n * EPS[np.dtype(dtype)] * np.abs(np.tril(want)).max()
    # deletion on a view
    ld, a = ref.case_delete(n, dtype)
    lp, lv = place(ld, layout)
    lp0 = lp.clone()
    F.ldlt_delete_rows_and_cols_clobber(lv, [2, nb])
    F.synchronize()
    guard_intact(lp, lp0, view_box(ld.shape, layout, dtype), "LD")
    keep = np.setdiff1d(np.arange(n), [2, nb])
    got = lv.cpu().numpy()[:n - 2, :n - 2]
    assert np.abs(ref.ldlt_product(got) - a[np.ix_(keep, keep)]).max() <= ref.residual_bound(n, a, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_negative_row_stride_through_the_c_entry(dtype):
    """L and W stored with their rows in reverse order: the views start at the last stored row and step backwards"""
    F = init_gpu()
    nb, rc = shape(dtype)
    n, r = nb + 2, 3
    f, w, alpha, _, _, want = ref_update(n, r, dtype, False, False)
    dl, dw, da = to_dev(f[::-1]), to_dev(w[::-1]), dvec(alpha)
    isz = np.dtype(dtype).itemsize
    fn = getattr(F.lib(), f"faer_hip_llt_rank_r_update_clobber_{'f64' if isz == 8 else 'f32'}")
    fn.restype = F.LltStatus
    st = fn(F.MatMut(dl.data_ptr() + (n - 1) * isz, n, n, -1, n), F.MatMut(dw.data_ptr() + (n - 1) * isz, n, r, -1, n), F.VecMut(da.data_ptr(), r, 1))
    assert st.tag == 0
    got = to_host(dl)[::-1]
    assert np.array_equal(bits(np.ascontiguousarray(np.triu(got, 1))), bits(np.ascontiguousarray(np.triu(f, 1))))
    assert np.abs(np.tril(got) - np.tril(want)).max() <= 4 * n * EPS[np.dtype(dtype)] * np.abs(np.tril(want)).max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("host", ["l", "w", "alpha", "all"])
def test_host_operands(host, dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    n, r = nb + 5, rc + 2
    for ldlt in (False, True):
        f, w, alpha, _, _, _ = ref_update(n, r, dtype, ldlt, False)
        base = gpu_update(F, f, w, alpha, ldlt)
        hp, hl = place_host(f, "sub")
        hp0 = hp.copy()
        l = hl if host in ("l", "all") else to_dev(f)
        ww = w.copy(order="F") if host in ("w", "all") else to_dev(w)
        aa = alpha.copy() if host in ("alpha", "all") else dvec(alpha)
        (F.ldlt_rank_r_update_clobber if ldlt else F.llt_rank_r_update_clobber)(l, ww, aa)
        if host in ("l", "all"):
            guard_intact(hp, hp0, view_box(f.shape, "sub", dtype), "host L")
            got = np.array(hl)
        else:
            got = to_host(l)
        assert np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(base))), (host, ldlt)
    ld, _ = ref.case_delete(n, dtype)
    dl = to_dev(ld)
    F.ldlt_delete_rows_and_cols_clobber(dl, [1, nb + 1])
    hl = ld.copy(order="F")
    F.ldlt_delete_rows_and_cols_clobber(hl, [1, nb + 1])
    assert np.array_equal(bits(hl[:n - 2, :n - 2].copy()), bits(to_host(dl)[:n - 2, :n - 2].copy()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["llt", "delete"])
def test_poisoned_pool(what, dtype):
    """every arena slice is written before it is read: the outputs do not depend on what the pool held"""
    F = init_gpu()
    nb, rc = shape(dtype)
    n, r = 2 * nb + 1, 2 * rc + 1
    f, w, alpha, _, _, _ = ref_update(n, r, dtype, False, False)
    ld, _ = ref.case_delete(n, dtype)

    def call():
        if what == "llt":
            return gpu_update(F, f, w, alpha, False)
        dl = to_dev(ld)
        F.ldlt_delete_rows_and_cols_clobber(dl, [0, 3, nb, n - 1])
        return to_host(dl)[:n - 4, :n - 4].copy()

    try:
        F.debug_scratch_fill(-1)
        base = call()
        F.debug_scratch_fill(0xFF)
        ff = call()
        count, nbytes = F.debug_scratch_fill_stats()
        F.debug_scratch_fill(0x7F)
        sf = call()
    finally:
        F.debug_scratch_fill(-1)
    assert count > 0 and nbytes > 0
    assert np.array_equal(bits(base), bits(ff)) and np.array_equal(bits(base), bits(sf))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_order(dtype):
    F = init_gpu()
    nb, rc = shape(dtype)
    n, r = 2 * nb + 1, rc + 1
    f, w, alpha, _, _, _ = ref_update(n, r, dtype, False, False)
    f2, w2, alpha2, _, _, _ = ref_update(n, r, dtype, False, True)

    def fn(bufs):
        return {"index": F.llt_rank_r_update_clobber(bufs["l"], bufs["w"], bufs["alpha"], raise_on_error=False), "l": bufs["l"]}

    good = {"l": to_dev(f), "w": to_dev(w), "alpha": dvec(alpha)}
    stale = {"l": to_dev(f2), "w": to_dev(w2), "alpha": dvec(alpha2)}
    expected, got = ordered_call(fn, good, stale)
    assert expected["index"] is None
    same_result(expected, got, "llt rank-r update")
