"""The complex triangular inverse on the device (csrc/ctrtri.hip): c32 / c64, lower / upper, unit or not.

Sizes sit around the leaf edge E and its sub-block edges (read from debug_ctrtri_shape) and around the first two levels above the leaf.
Every call gets a destination pre-filled with a NaN-payload sentinel and a source whose unread parts are NaN; what must stay untouched
is compared bit for bit.  The residual (complex_tri_inverse_ref.residual) is held against the numpy restatement of the reference's
recursion on the same input in the same precision: residual_gpu <= FACTOR * max(residual_ref, eps), FACTOR from the ratios recorded in
profiles/complex_tri_inverse_error.txt (see complex_tri_inverse_ref.FACTOR).  Equality in the exact case is equality of values: the
inverse is a mathematical object without signed zeros, and which zero a schedule leaves in the vanishing part of an entry is its own
business.  A row-major destination is compared with the column-major one by the residual bound, not bit for bit: the complex GEMM runs
such a destination transposed, which swaps the order of the two products summed into an imaginary part."""
import numpy as np
import pytest

import complex_cases as cc
import complex_tri_inverse_ref as ref
from gpu_util import fa, init_gpu, ordered_call, to_dev, to_host

pytestmark = pytest.mark.gpu

DTYPES = (np.complex64, np.complex128)
# Sizes by name: E and the sub-block edge are read from the library inside the tests (loading it while the module is imported would
# put its HIP runtime into the process before torch's).  "sub" stands for every sub-block edge +- 1.
SIZE_NAMES = ("1", "2", "sub", "E-1", "E", "E+1", "2E", "2E+1", "3E+5", "4E+E/2")


def shape(dtype):
    return fa().debug_ctrtri_shape(dtype)


def named_sizes(name, dtype):
    e, sub = shape(dtype)
    sb = e // sub
    if name == "sub":
        out = sorted({k * sb + d for k in range(1, sub) for d in (-1, 1)})
    else:
        out = [{"1": 1, "2": 2, "E-1": e - 1, "E": e, "E+1": e + 1, "2E": 2 * e, "2E+1": 2 * e + 1, "3E+5": 3 * e + 5, "4E+E/2": 4 * e + e // 2}[name]]
    assert set(out) <= set(ref.sizes(e, sub))
    return out


def invert(F, tp, triangle, unit, order="F"):
    """the call on device operands: source `tp` in `order`, destination a column-major sentinel; returns the destination on the host"""
    n = tp.shape[0]
    dw = to_dev(ref.sentinel(n, tp.dtype))
    F.inverse_triangular_in_place(dw, to_dev(tp, order), upper=triangle == "upper", unit=unit)
    return to_host(dw)


def assert_untouched(w, triangle, unit, what):
    n = w.shape[0]
    keep = ~ref.written_mask(n, triangle, unit)
    s = ref.sentinel(n, w.dtype)
    assert ref.same_bits(np.where(keep, w, 0), np.where(keep, s, 0)), what
    assert np.isfinite(w[~keep]).all(), what


def within_bound(t, w, r_ref, triangle, unit, what):
    r = ref.residual(t, w, triangle, unit)
    y = ref.yardstick(r_ref, t.dtype)
    print(f"ctrtri-ratio {what}: r_gpu {r:.3e} r_ref {r_ref:.3e} ratio {r / y:.3f}")
    assert r <= ref.FACTOR * y, (what, r, r_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_residual_and_untouched_parts(size, dtype):
    F = init_gpu()
    for n in named_sizes(size, dtype):
        for triangle, unit in ref.VARIANTS:
            what = f"n={n} {triangle} unit={unit} {np.dtype(dtype).name}"
            t, tp, _, r_ref = ref.case(n, dtype, triangle, unit)
            w = invert(F, tp, triangle, unit)
            assert_untouched(w, triangle, unit, what)
            within_bound(t, w, r_ref, triangle, unit, what)


def test_every_size_has_a_name():
    init_gpu()
    for dtype in DTYPES:
        assert sorted(n for name in SIZE_NAMES for n in named_sizes(name, dtype)) == ref.sizes(*shape(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact(dtype):
    F = init_gpu()
    e = shape(dtype)[0]
    for n in (e + 1, 3 * e + 5):
        for triangle, unit in ref.VARIANTS:
            t, want = ref.exact_case(n, dtype, triangle, unit)
            w = invert(F, cc.tri_poisoned(t, triangle, unit), triangle, unit)
            assert_untouched(w, triangle, unit, (n, triangle, unit))
            m = ref.written_mask(n, triangle, unit)
            assert np.array_equal(w[m], want[m]), (n, triangle, unit)


def solver(F, triangle, unit):
    return {("lower", False): F.solve_lower_triangular_in_place, ("upper", False): F.solve_upper_triangular_in_place,
            ("lower", True): F.solve_unit_lower_triangular_in_place, ("upper", True): F.solve_unit_upper_triangular_in_place}[(triangle, unit)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_consistent_with_the_solve(dtype):
    """X = solve(T, B) and W B (the product in clongdouble) differ by d with |T d| <= |T W B - B| + |T X - B|: the inverse's part is at
    most FACTOR * yardstick * (|T||W|)|B|, the solve's C_TRI_COMPLEX n eps (|T||X| + |B|) (complex_cases.py)"""
    F = init_gpu()
    e = shape(dtype)[0]
    for n in (e + 1, 3 * e + 5):
        for triangle, unit in ref.VARIANTS:
            t, tp, _, r_ref = ref.case(n, dtype, triangle, unit)
            b = cc.crandn(np.random.default_rng(n + 17), n, 7, dtype)
            w = ref.effective(invert(F, tp, triangle, unit), triangle, unit)
            dx = to_dev(b)
            solver(F, triangle, unit)(to_dev(tp), dx)
            x = to_host(dx)
            te, we, be, xe = cc.ext(ref.effective(t, triangle, unit)), cc.ext(w), cc.ext(b), cc.ext(x)
            lhs = np.abs(te @ (we @ be - xe))
            bound = (ref.FACTOR * ref.yardstick(r_ref, dtype) * (np.abs(te) @ np.abs(we) @ np.abs(be))
                     + cc.C_TRI_COMPLEX * n * cc.ceps(dtype) * (np.abs(te) @ np.abs(xe) + np.abs(be)))
            assert (lhs <= bound).all(), (n, triangle, unit, float((lhs / bound).max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_views(dtype):
    import torch

    F = init_gpu()
    n = 2 * shape(dtype)[0] + 1
    isz = np.dtype(dtype).itemsize
    for triangle, unit in ref.VARIANTS:
        upper = triangle == "upper"
        t, tp, _, r_ref = ref.case(n, dtype, triangle, unit)
        base = invert(F, tp, triangle, unit)
        what = (triangle, unit)
        # row-major source, column-major destination
        assert ref.same_bits(invert(F, tp, triangle, unit, "C"), base), what
        # row-major destination: by the residual bound (module docstring), untouched parts bit for bit
        dw = to_dev(ref.sentinel(n, dtype), "C")
        F.inverse_triangular_in_place(dw, to_dev(tp, "C"), upper=upper, unit=unit)
        w = to_host(dw)
        assert_untouched(w, triangle, unit, what)
        within_bound(t, w, r_ref, triangle, unit, f"row-major dst n={n} {triangle} unit={unit} {np.dtype(dtype).name}")
        # padded leading dimension, then an offset block of a larger buffer: the parent outside the view keeps its sentinel
        for r0, c0 in ((0, 0), (5, 3)):
            ps = to_dev(ref.sentinel(2 * n + 8, dtype))
            pt = to_dev(np.full((2 * n + 8, 2 * n + 8), np.nan + 1j * np.nan, dtype=dtype))
            pt[r0 + 1:r0 + 1 + n, c0 + 2:c0 + 2 + n] = to_dev(tp)
            F.inverse_triangular_in_place(ps[r0:r0 + n, c0:c0 + n], pt[r0 + 1:r0 + 1 + n, c0 + 2:c0 + 2 + n], upper=upper, unit=unit)
            got = to_host(ps)
            assert ref.same_bits(got[r0:r0 + n, c0:c0 + n], base), (what, r0, c0)
            outside = np.ones(got.shape, bool)
            outside[r0:r0 + n, c0:c0 + n] = False
            s = ref.sentinel(2 * n + 8, dtype)
            assert ref.same_bits(np.where(outside, got, 0), np.where(outside, s, 0)), (what, r0, c0)
        # reversed rows and columns: the flipped matrices on the device, handed over with negative strides
        dt_, dw = to_dev(np.array(tp)[::-1, ::-1]), to_dev(ref.sentinel(n, dtype))
        last = lambda d: d.data_ptr() + ((n - 1) * d.stride(0) + (n - 1) * d.stride(1)) * isz  # noqa: E731
        name = f"libfaer_v0_23_inverse_{'unit_' if unit else ''}triangular_{triangle}_in_place_{'c32' if isz == 8 else 'c64'}"
        getattr(F.lib(), name)(F.MatMut(last(dw), n, n, -dw.stride(0), -dw.stride(1)), F.MatRef(last(dt_), n, n, -dt_.stride(0), -dt_.stride(1)),
                               F.PAR_SEQ)
        assert ref.same_bits(np.array(to_host(dw))[::-1, ::-1], base), what
        del dt_, dw
        # host operands (staged through the scratch pool), then host operands with negative strides (packed element by element)
        hw = ref.sentinel(n, dtype)
        F.inverse_triangular_in_place(hw, np.array(tp), upper=upper, unit=unit)
        assert ref.same_bits(hw, base), what
        hw, ht = ref.sentinel(n, dtype), np.array(np.array(tp)[::-1, ::-1], order="F")
        F.inverse_triangular_in_place(hw[::-1, ::-1], ht[::-1, ::-1], upper=upper, unit=unit)
        assert ref.same_bits(hw[::-1, ::-1], base), what
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_pool(dtype):
    """the product buffer of the levels is a slice of the call's arena and host operands are staged through the pool: filled with 0xFF
    and 0x7F bytes first, the results are those of the unpoisoned run bit for bit, and buffers were in fact filled"""
    F = init_gpu()
    n = 3 * shape(dtype)[0] + 5

    def run():
        out = []
        for triangle, unit in ref.VARIANTS:
            _, tp, _, _ = ref.case(n, dtype, triangle, unit)
            out.append(invert(F, tp, triangle, unit))
            hw = ref.sentinel(n, dtype)
            F.inverse_triangular_in_place(hw, np.array(tp), upper=triangle == "upper", unit=unit)
            out.append(hw)
        return out

    try:
        want = run()
        for byte in (0xFF, 0x7F):
            F.debug_scratch_fill(byte)
            got = run()
            assert F.debug_scratch_fill_stats()[0] > 0, byte
            for k, (g, w) in enumerate(zip(got, want)):
                assert ref.same_bits(g, w), (byte, k)
    finally:
        F.debug_scratch_fill(-1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_caller_stream(dtype):
    """on a non-blocking torch stream between a producer that writes T and a consumer that reads W (gpu_util.ordered_call): a call
    that ran ahead of the producer would invert the stale matrix, one that returned before its work was in the stream would hand the
    consumer an unfinished W"""
    F = init_gpu()
    n = 3 * shape(dtype)[0] + 5
    _, tp, _, _ = ref.case(n, dtype, "lower", False)
    _, stale, _, _ = ref.case(n, dtype, "upper", False)

    def fn(b):
        F.inverse_triangular_in_place(b["w"], b["t"], upper=False, unit=False)
        return {"w": b["w"]}

    s = ref.sentinel(n, dtype)
    expected, got = ordered_call(fn, {"t": np.array(tp), "w": s}, {"t": np.array(stale.T, order="F") * 3, "w": s})
    assert_untouched(expected["w"], "lower", False, "default stream")
    assert ref.same_bits(got["w"], expected["w"])
