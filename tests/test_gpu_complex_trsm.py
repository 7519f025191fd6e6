"""Complex triangular solves on the device (csrc/ctrsm.hip): componentwise backward error against the bound of complex_cases.py for
every variant, conjugation and storage order of T; exact Gaussian-integer solves (the two conjugations give different answers);
locality of a zero pivot; and the staging buffers of the complex entry points on a poisoned scratch pool."""
import numpy as np
import pytest

import complex_cases as cc
from gpu_util import fa, init_gpu, to_dev, to_host

pytestmark = pytest.mark.gpu


def solver(F, triangle, unit):
    return {("lower", False): F.solve_lower_triangular_in_place, ("upper", False): F.solve_upper_triangular_in_place,
            ("lower", True): F.solve_unit_lower_triangular_in_place, ("upper", True): F.solve_unit_upper_triangular_in_place}[(triangle, unit)]


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("t_order", ["F", "C"])
@pytest.mark.parametrize("nrhs", cc.TRSM_NRHS)
@pytest.mark.parametrize("n", cc.TRSM_SIZES)
def test_backward_error(n, nrhs, t_order, dtype):
    F = init_gpu()
    for triangle, unit in cc.TRSM_VARIANTS:
        t, b = cc.trsm_case(n, nrhs, dtype, triangle, unit)
        dt = to_dev(cc.tri_poisoned(t, triangle, unit), t_order)  # the other triangle (and a unit diagonal) is never read
        for conj in (False, True):
            dx = to_dev(b)
            solver(F, triangle, unit)(dt, dx, conj=conj)
            q = cc.tri_backward_error(t, to_host(dx), b, conj)
            print(f"n={n} nrhs={nrhs} {triangle} unit={unit} conj={conj} T {t_order} {np.dtype(dtype).name}: {q:.3f} of the bound")
            assert q <= 1.0, (triangle, unit, conj, q)


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("n", [40, 130])
def test_exact(n, dtype):
    F = init_gpu()
    for triangle, unit in cc.TRSM_VARIANTS:
        for conj in (False, True):
            t, b, x0 = cc.exact_trsm_case(n, 33, dtype, triangle, unit, conj)
            dt = to_dev(cc.tri_poisoned(t, triangle, unit))
            dx = to_dev(b, "C")
            solver(F, triangle, unit)(dt, dx, conj=conj)
            assert np.array_equal(to_host(dx), x0), (triangle, unit, conj)
            dy = to_dev(b)
            solver(F, triangle, unit)(dt, dy, conj=not conj)  # the other conjugation solves another system
            assert not np.array_equal(to_host(dy), x0), (triangle, unit, conj)


@pytest.mark.parametrize("dtype", cc.CDTYPES)
def test_zero_pivot_is_local(dtype):
    F = init_gpu()
    n, bad = 300, 200
    t, b = cc.trsm_case(n, 33, dtype, "lower", False)
    t = np.array(t)
    t[bad, bad] = 0
    dx = to_dev(b)
    F.solve_lower_triangular_in_place(to_dev(t), dx)
    x = to_host(dx)
    assert np.isfinite(x[:bad]).all()
    assert not np.isfinite(x[bad]).any()
    # the rows before the pivot are the solution of the leading block
    assert cc.tri_backward_error(t[:bad, :bad], x[:bad], b[:bad], False) <= 1.0


def test_poisoned_pool():
    """host operands (every one is staged through the scratch pool) after the pool has been filled with 0xFF and 0x7F bytes: the
    results are those of the unpoisoned run, and buffers were in fact filled"""
    F = init_gpu()
    m, n, k = 129, 127, 130
    a, b, c0, _, _ = cc.matmul_case(m, n, k, np.complex128)
    t, rhs = cc.trsm_case(129, 33, np.complex64, "upper", False)
    tp = cc.tri_poisoned(t, "upper", False)

    def run():
        c = np.full((m, n), np.nan + 1j * np.nan, order="F")
        F.matmul(c, F.ACCUM_REPLACE, np.array(a), np.array(b), 2 - 1j)
        x = np.array(rhs)
        F.solve_upper_triangular_in_place(tp, x, conj=True)
        return c, x

    try:
        c_ref, x_ref = run()
        assert np.isfinite(c_ref).all() and np.isfinite(x_ref).all()
        ref, bound = cc.matmul_ref_and_bound(m, n, k, np.complex128, "replace", 2 - 1j)
        assert (np.abs(cc.ext(c_ref) - ref) <= bound).all()
        assert cc.tri_backward_error(t, x_ref, rhs, True) <= 1.0
        for byte in (0xFF, 0x7F):
            F.debug_scratch_fill(byte)
            c, x = run()
            assert F.debug_scratch_fill_stats()[0] > 0, byte
            assert np.array_equal(c, c_ref) and np.array_equal(x, x_ref), byte
    finally:
        F.debug_scratch_fill(-1)
