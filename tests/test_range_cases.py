"""The references alone at the ends of the floating-point range (no GPU): for every family, case, dtype and scale of tests/range_cases.py
the scaled input and the reference's output hold only zeros and normal numbers (cap_ok), and reference(2^k A) agrees with the rescaled
reference(A) within the bound tests/test_gpu_range_edges.py holds the kernels to -- so a kernel that misses that bound at some scale
is wrong, not the reference."""
import numpy as np
import pytest

import range_cases as rc

PARAMS = [pytest.param(f, c, s, dt, id=f"{f}-{c}-{s}-{np.dtype(dt).name}".replace(" ", "")) for f in rc.CASES for c, s in rc.family_cases(f)
          for dt in rc.DTYPES]


def check_family_case(oracle, family, case, strat, dtype, a=None):
    a = rc.make_input(family, case, dtype) if a is None else a
    e_in = rc.IN_EXP[family]
    p0, x0 = rc.reference(oracle, family, a, strat)
    r = rc.unscaled_parts(p0, 0)
    for k in rc.K[family][np.dtype(dtype)]:
        ak = rc.scaled(a, k, e_in)
        assert rc.cap_ok(ak), ("input", k)
        assert np.array_equal(rc.unscale(ak, k, e_in), a.astype(np.float64)), ("the scaling is not exact", k)
        pk, xk = rc.reference(oracle, family, ak, strat)
        assert all(rc.cap_ok_taus(np.asarray(x).astype(dtype)) for x, _ in pk.values()), ("output", k)
        rc.same_exact(x0, xk)
        g = rc.unscaled_parts(pk, k)
        if family == "lu":
            rc.compare_lu(g, r, a, x0["perm"])
        else:
            rc.COMPARE[family](g, r, a)


@pytest.mark.parametrize("family,case,strat,dtype", PARAMS)
def test_reference_is_scale_equivariant_inside_the_tables(oracle, family, case, strat, dtype):
    check_family_case(oracle, family, case, strat, dtype)


def test_reference_llt_at_the_look_ahead_size(oracle):
    check_family_case(oracle, "llt", rc.LLT_LOOKAHEAD_N, None, np.float64)


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_reference_colpiv_qr_graded_columns(oracle, dtype):
    """columns scaled individually over the whole table range: inputs and outputs stay normal, the column norms are distinct by
    more than a factor of two (no pivot ties)"""
    kx = rc.GRADED_KX[np.dtype(dtype)]
    a, g, c = rc.graded_columns(300, 40, dtype, kx)
    assert rc.cap_ok(a)
    nrm = np.sort(np.linalg.norm(g.astype(np.float64), axis=0) * c)
    assert (nrm[1:] / nrm[:-1]).min() >= 2.0
    parts, exact = rc.reference(oracle, "colpiv_qr", a)
    assert rc.outputs_cap_ok(parts)
    # the pivot order is the order of the column norms, largest first
    assert np.array_equal(exact["perm"], np.argsort(-np.linalg.norm(g.astype(np.float64), axis=0) * c))


def test_reference_qr_rank_deficient(oracle):
    """the fp32 case of the general QR path: the same rank and pattern of skipped reflectors at every scale, nothing subnormal"""
    a = rc.rank_deficient(*rc.QR_DEFICIENT, np.float32)
    m, n = a.shape

    def run(x):
        ref, rh = x.copy(order="F"), np.zeros((32, n), dtype=np.float32, order="F")
        return oracle.qr_in_place(ref, rh), ref, rh

    rk0, _, rh0 = run(a)
    assert rc.QR_DEFICIENT[2] <= rk0 < n
    for k in rc.K["qr_deficient"][rc.F32]:
        ak = rc.scaled(a, k)
        assert rc.cap_ok(ak)
        rk, ref, rh = run(ak)
        assert rk == rk0 and np.array_equal(np.isinf(rh), np.isinf(rh0))
        assert rc.cap_ok(ref) and rc.cap_ok_taus(rh), k


def test_tables_cross_the_thresholds():
    for dt, lim in ((rc.F64, 511), (rc.F32, 63)):
        lo, _, _, hi = rc.GENERAL[dt]
        assert lo <= -lim - 20 and hi >= lim + 20  # entries of relative size 2^+-20 are still beyond the accumulator switch
    lo, ml, mh, hi = rc.CHOLESKY[rc.F64]
    assert 4.0 ** hi * 100 > 1e280 * 3100 and 4.0 ** lo * 2 * 3100 < 1e-280  # pivots of every case beyond the v_rsq_f64 window
    assert 1e-280 < 4.0 ** ml and 4.0 ** mh * 2 * 3100 < 1e280


def test_cap_ok():
    t = np.finfo(np.float32).tiny
    assert rc.cap_ok(np.array([0.0, -0.0, t, -3.0, 1e38], dtype=np.float32))
    assert not rc.cap_ok(np.array([t / 2], dtype=np.float32))
    assert not rc.cap_ok(np.array([np.inf])) and not rc.cap_ok(np.array([np.nan]))
    assert rc.cap_ok_taus(np.array([np.inf, 0.5])) and not rc.cap_ok_taus(np.array([-np.inf]))
