"""Complex products on the device (csrc/cgemm.hip): parity with numpy in clongdouble inside the componentwise bound of
complex_cases.py, exact Gaussian-integer products for every conjugation, DstKind, stride form and FaerBlock combination (a sign or
conjugation slip, a wrong mask or a read of an excluded entry shows as a wrong integer or a NaN), and one product on a non-blocking
caller stream.  "Exact" results are compared as values (a zero may carry either sign); entries that must not be written are compared
bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest

import complex_cases as cc
from gpu_util import fa, init_gpu, ordered_call, same_result, to_dev, to_host

pytestmark = pytest.mark.gpu


def cbits(x):
    """a complex numpy array as integers: shape + (2,), the bit patterns of re and im"""
    x = np.ascontiguousarray(x)
    real, integer = (np.float64, np.int64) if x.dtype == np.complex128 else (np.float32, np.int32)
    return x.view(real).reshape(x.shape + (2,)).view(integer)


def sentinel(m, n, dtype):
    """finite, non-integer, all different: what an untouched entry of dst has to come back as"""
    i, j = np.indices((m, n))
    return np.asarray((1000.5 + i + 0.25 * j) - 1j * (2000.75 + 3 * i + j), dtype=dtype, order="F")


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("layout", ["FFF", "CFF", "FCF", "CCC"])
@pytest.mark.parametrize("m,n,k", cc.MATMUL_SHAPES)
def test_matmul_parity(m, n, k, layout, dtype):
    F = init_gpu()
    a, b, c0, _, _ = cc.matmul_case(m, n, k, dtype)
    da, db = to_dev(a, layout[0]), to_dev(b, layout[1])
    for mode, alpha in cc.MATMUL_MODES:
        add = mode == "add"
        dc = to_dev(c0 if add else np.full((m, n), np.nan + 1j * np.nan, dtype=dtype), layout[2])
        F.matmul(dc, F.ACCUM_ADD if add else F.ACCUM_REPLACE, da, db, alpha)
        got = to_host(dc)
        ref, bound = cc.matmul_ref_and_bound(m, n, k, dtype, mode, alpha)
        err = np.abs(cc.ext(got) - ref)
        assert np.isfinite(got).all() and (err <= bound).all(), (mode, float(np.max(err - bound)))


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("m,n,k", [(17, 33, 256), (130, 70, 129)])
def test_gemm_conjugations_exact(m, n, k, dtype):
    F = init_gpu()
    rng = np.random.default_rng(m + n + k)
    a, b, c0 = cc.gauss_int(rng, m, k, dtype), cc.gauss_int(rng, k, n, dtype), cc.gauss_int(rng, m, n, dtype)
    da, db = to_dev(a), to_dev(b, "C")
    for cl, cr in itertools.product((False, True), repeat=2):
        want = (np.conj(a) if cl else a).astype(np.complex128) @ (np.conj(b) if cr else b).astype(np.complex128)
        dc = to_dev(np.full((m, n), np.nan + 1j * np.nan, dtype=dtype))  # Replace into NaN
        F.gemm(dc, F.DST_FULL, F.ACCUM_REPLACE, da, db, 1 - 2j, conj_lhs=cl, conj_rhs=cr)
        assert np.array_equal(to_host(dc), ((1 - 2j) * want).astype(dtype)), (cl, cr)
        dc = to_dev(c0)
        F.gemm(dc, F.DST_FULL, F.ACCUM_ADD, da, db, -1j, conj_lhs=cl, conj_rhs=cr)
        assert np.array_equal(to_host(dc), (c0 - 1j * want).astype(dtype)), (cl, cr)


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("n", [17, 130])
@pytest.mark.parametrize("kind", ["lower", "upper"])
def test_gemm_dst_kind_leaves_the_other_triangle(kind, n, dtype):
    F = init_gpu()
    rng = np.random.default_rng(n)
    k = 40
    a, b = cc.gauss_int(rng, n, k, dtype), cc.gauss_int(rng, k, n, dtype)
    want = (2 + 1j) * (a.astype(np.complex128) @ np.conj(b).astype(np.complex128))
    written = cc.block_mask(kind, n, n)
    for order in ("F", "C"):
        c0 = sentinel(n, n, dtype)
        for add in (False, True):
            dc = to_dev(c0, order)
            F.gemm(dc, F.DST_LOWER if kind == "lower" else F.DST_UPPER, F.ACCUM_ADD if add else F.ACCUM_REPLACE, to_dev(a), to_dev(b),
                   2 + 1j, conj_rhs=True)
            got = to_host(dc)
            exp = (want + (c0 if add else 0)).astype(dtype)
            assert np.array_equal(got[written], exp[written]), (order, add)
            assert np.array_equal(cbits(got)[~written], cbits(c0)[~written]), (order, add)


@pytest.mark.parametrize("dtype", cc.CDTYPES)
def test_gemm_generic_and_reversed_strides_exact(dtype):
    """device views with non-unit strides and flipped rows (as test_matmul_negative_and_generic_strides), then hand-made views with
    negative device strides, then host views with negative strides"""
    F = init_gpu()
    rng = np.random.default_rng(5)
    m, k, n = 70, 90, 50
    a, b = cc.gauss_int(rng, m, k, dtype), cc.gauss_int(rng, k, n, dtype)
    want = np.conj(a).astype(np.complex128) @ b.astype(np.complex128)
    big_a, big_b = to_dev(np.zeros((2 * m, 2 * k), dtype=dtype)), to_dev(np.zeros((2 * k, 2 * n), dtype=dtype))
    big_a[::2, ::2] = to_dev(a)
    big_b[::2, ::2] = to_dev(b)
    big_c = to_dev(sentinel(3 * m, 2 * n, dtype))
    vc = big_c[1::3, ::2]
    F.gemm(vc, F.DST_FULL, F.ACCUM_REPLACE, big_a[::2, ::2].flip(0), big_b[::2, ::2], 1.0, conj_lhs=True)
    got = to_host(big_c)
    assert np.array_equal(got[1::3, ::2], want[::-1].astype(dtype))
    untouched = np.ones(got.shape, bool)
    untouched[1::3, ::2] = False
    assert np.array_equal(cbits(got)[untouched], cbits(sentinel(3 * m, 2 * n, dtype))[untouched])
    # negative device strides: rows of a reversed, columns of b reversed
    da, db, dc = to_dev(a), to_dev(b), to_dev(np.zeros((m, n), dtype=dtype))
    isz = np.dtype(dtype).itemsize
    va = F.MatRef(da.data_ptr() + (m - 1) * da.stride(0) * isz, m, k, -da.stride(0), da.stride(1))
    vb = F.MatRef(db.data_ptr() + (n - 1) * db.stride(1) * isz, k, n, db.stride(0), -db.stride(1))
    suf, ct, _ = F._dtype_suffix(dc)
    al = ct(1j)
    getattr(F.lib(), f"libfaer_v0_23_matmul_{suf}")(F._mat(dc, F.MatMut), C.c_int(F.ACCUM_REPLACE), va, vb, C.byref(al), F.PAR_SEQ)
    assert np.array_equal(to_host(dc), (1j * (a[::-1].astype(np.complex128) @ b[:, ::-1].astype(np.complex128))).astype(dtype))
    # host operands with negative strides (staged element by element)
    hc = np.zeros((m, n), dtype=dtype, order="F")
    F.gemm(hc[::-1], F.DST_FULL, F.ACCUM_REPLACE, a[::-1, ::-1], b[::-1], 1.0, conj_lhs=True)
    assert np.array_equal(hc[::-1], (np.conj(a[::-1, ::-1]).astype(np.complex128) @ b[::-1].astype(np.complex128)).astype(dtype))


def tri_product_case(F, n, dtype, combos, seed):
    """matmul_triangular for each (dst, lhs, rhs) block combination in `combos`: operands NaN outside their block, exact result"""
    rng = np.random.default_rng(seed)
    a, b, c0 = cc.gauss_int(rng, n, n, dtype), cc.gauss_int(rng, n, n, dtype), sentinel(n, n, dtype)
    dev_a = {s: to_dev(cc.block_poisoned(a, s)) for s in cc.BLOCKS}
    dev_b = {s: to_dev(cc.block_poisoned(b, s), "C") for s in cc.BLOCKS}
    eff_a = {s: cc.block_effective(a, s).astype(np.complex128) for s in cc.BLOCKS}
    eff_b = {s: cc.block_effective(b, s).astype(np.complex128) for s in cc.BLOCKS}
    dc0 = to_dev(c0)
    for idx, (cs, as_, bs) in enumerate(combos):
        add = idx % 2 == 0
        alpha = (-1 + 2j) if add else (2 - 1j)
        # the dst block of matmul_triangular is written where the block's mask holds (a unit dst keeps its diagonal: triangular.rs)
        written = cc.block_mask(cs, n, n)
        dc = dc0.clone()
        if not add:
            dc[to_dev(written)] = complex(np.nan, np.nan)  # Replace never reads dst
        F.matmul_triangular(dc, cs, F.ACCUM_ADD if add else F.ACCUM_REPLACE, dev_a[as_], as_, dev_b[bs], bs, alpha)
        got = to_host(dc)
        exp = (alpha * (eff_a[as_] @ eff_b[bs]) + (c0 if add else 0)).astype(dtype)
        assert np.array_equal(got[written], exp[written]), (cs, as_, bs, add)
        assert np.array_equal(cbits(got)[~written], cbits(c0)[~written]), (cs, as_, bs, add)


@pytest.mark.parametrize("dtype", cc.CDTYPES)
def test_matmul_triangular_every_combination(dtype):
    F = init_gpu()
    tri_product_case(F, 33, dtype, list(itertools.product(cc.BLOCKS, repeat=3)), 33)


# every kind once per position, across the 128 edge
COMBOS_130 = [("rect", "lower", "upper"), ("lower", "rect", "rect"), ("upper", "unit_lower", "strict_upper"),
              ("strict_lower", "strict_lower", "lower"), ("strict_upper", "upper", "unit_upper"), ("unit_lower", "strict_upper", "unit_lower"),
              ("unit_upper", "unit_upper", "strict_lower"), ("rect", "unit_lower", "unit_upper"), ("lower", "lower", "lower"),
              ("upper", "upper", "upper"), ("rect", "strict_lower", "strict_upper"), ("lower", "unit_upper", "rect")]


@pytest.mark.parametrize("dtype", cc.CDTYPES)
def test_matmul_triangular_across_the_tile_edge(dtype):
    F = init_gpu()
    for pos in range(3):
        assert {c[pos] for c in COMBOS_130} == set(cc.BLOCKS)
    tri_product_case(F, 130, dtype, COMBOS_130, 130)


def test_matmul_on_a_caller_stream():
    """a c64 product queued on a non-blocking caller stream between a producer and a consumer on that stream (gpu_util.ordered_call)"""
    F = init_gpu()
    m, n, k = 300, 200, 1000
    a, b, c0, _, _ = cc.matmul_case(m, n, k, np.complex128)
    good = {"a": np.array(a), "b": np.array(b), "c": np.full((m, n), np.nan + 1j * np.nan, order="F")}
    stale = {"a": np.zeros_like(a), "b": np.zeros_like(b), "c": np.array(c0)}

    def fn(bufs):
        F.matmul(bufs["c"], F.ACCUM_REPLACE, bufs["a"], bufs["b"], 2 - 1j)
        return {"c": bufs["c"]}

    expected, got = ordered_call(fn, good, stale)
    same_result(expected, got, "c64 matmul on a caller stream")
    ref, bound = cc.matmul_ref_and_bound(m, n, k, np.complex128, "replace", 2 - 1j)
    assert (np.abs(cc.ext(got["c"]) - ref) <= bound).all()
