"""GPU tests of the Bunch-Kaufman factorization (include/faer_hip.h section 2g, csrc/lblt.hip) against tests/lblt_ref.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import lblt_ref as ref
from gpu_util import EPS, guard_intact, init_gpu, place, same_bits, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lblt_cases.json")))
SIZES = [1, 2, 3, 5, 63, 64, 65, 66, 129, 130, 200]
STRATS = list(ref.STRATEGIES)
DTYPES = [np.float64, np.float32]
ITYPES = [np.uint32, np.uint64]


def tol(n, dtype, c=64):
    """the bound tests/test_gpu_extras.py uses for the ldlt reconstruction"""
    return c * max(n, 1) * EPS[np.dtype(dtype)]


def factor(F, a, strat, it=np.uint64, nan_upper=True):
    """factors the lower triangle of the numpy matrix `a` on the device; the strict upper triangle holds NaN on entry"""
    n = a.shape[0]
    a_in = np.array(a, order="F")
    if nan_upper:
        a_in[np.triu_indices(n, 1)] = np.nan
    d0 = to_dev(a_in)
    d = d0.clone()
    sub, pf, pb, cnt = F.lblt_factor_in_place(d, pivoting=ref.STRATEGIES[strat][0], index_dtype=it)
    F.synchronize()
    last = F.debug_lblt_last()
    import torch

    assert same_bits(torch.triu(d, 1), torch.triu(d0, 1)), "the strict upper triangle was written"
    return {"dev": d, "sub_dev": sub, "packed": to_host(d), "sub": to_host(sub), "pf": pf, "pb": pb, "count": cnt, "last": last}


def check_structure(r, n, strat):
    pf, pb = r["pf"].astype(np.int64), r["pb"].astype(np.int64)
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[pb], np.arange(n))
    if n > 0:
        assert round(np.linalg.det(np.eye(n)[pf])) == (-1) ** r["count"]
    sub, p = r["sub"], r["packed"]
    for j in range(n):
        if sub[j] != 0:
            assert j + 1 < n and sub[j + 1] == 0 and p[j + 1, j] == 0
    panels, leaf_rows, n2, syncs = r["last"]
    assert leaf_rows > 0 and (panels > 0) == (n > 64)
    assert n2 == np.count_nonzero(sub)
    if not ref.STRATEGIES[strat][1]:
        assert syncs == 0


def residual(r, a):
    """max |P A P^T - L B L^T| from the returned factors, in float64"""
    p = r["packed"].astype(np.float64)
    L = ref.unit_lower(p)
    pf = r["pf"].astype(np.int64)
    a64 = np.asarray(a, dtype=np.float64)
    return np.abs(a64[np.ix_(pf, pf)] - L @ ref.block_diag(np.diag(p), r["sub"].astype(np.float64)) @ L.T).max()


def check_accuracy(F, r, a, dtype):
    n = a.shape[0]
    amax = max(np.abs(a).max(), np.finfo(dtype).tiny)
    assert residual(r, a) <= tol(n, dtype) * amax
    out = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
    F.lblt_reconstruct(out, r["dev"], r["sub_dev"], r["pf"], r["pb"])
    got = to_host(out)
    il, iu = np.tril_indices(n), np.triu_indices(n, 1)
    assert (got[iu] == -7.5).all()
    assert np.abs(got[il].astype(np.float64) - a[il]).max() <= tol(n, dtype) * amax


def check_solve(F, r, a, dtype, seed):
    n = a.shape[0]
    a64 = np.asarray(a, dtype=np.float64)
    for k in (1, 7):
        b = np.asarray(np.random.default_rng(seed + k).standard_normal((n, k)), dtype=dtype, order="F")
        x = to_dev(b)
        F.lblt_solve_in_place(r["dev"], r["sub_dev"], r["pf"], r["pb"], x)
        xs = to_host(x).astype(np.float64)
        assert np.linalg.norm(a64 @ xs - b) <= tol(n, dtype) * np.linalg.norm(a64) * np.linalg.norm(xs), (k,)
    inv = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
    F.lblt_inverse(inv, r["dev"], r["sub_dev"], r["pf"], r["pb"])
    eye = to_dev(np.eye(n, dtype=dtype))
    F.lblt_solve_in_place(r["dev"], r["sub_dev"], r["pf"], r["pb"], eye)
    assert same_bits(inv, eye)


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("n", SIZES)
def test_gaussian(n, strat, dtype, it):
    F = init_gpu()
    a = np.asarray(ref.random_symmetric(n, 1000 + n), dtype=dtype)
    r = factor(F, a, strat, it)
    assert r["pf"].dtype == it
    check_structure(r, n, strat)
    check_accuracy(F, r, a, dtype)
    check_solve(F, r, a, dtype, n)
    plain = factor(F, a, strat, it, nan_upper=False)  # the content of the upper triangle does not matter
    il = np.tril_indices(n)
    assert np.array_equal(plain["packed"][il], r["packed"][il]) and np.array_equal(plain["sub"], r["sub"])
    assert np.array_equal(plain["pf"], r["pf"]) and plain["count"] == r["count"]


def special(kind, n):
    if kind == "kkt":
        return ref.kkt(n, 7)
    if kind == "spd":
        g = np.random.default_rng(n).standard_normal((n, n))
        return g @ g.T + n * np.eye(n)
    if kind == "identity":
        return np.eye(n)
    if kind == "zero":
        return np.zeros((n, n))
    a = ref.random_symmetric(n, 5)  # a zero row / column
    a[n // 2, :] = 0
    a[:, n // 2] = 0
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("n", [5, 66, 130])
@pytest.mark.parametrize("kind", ["kkt", "spd", "identity", "zero", "zero_row"])
def test_special_inputs(kind, n, strat, dtype):
    F = init_gpu()
    a = np.asarray(special(kind, n), dtype=dtype)
    r = factor(F, a, strat)
    check_structure(r, n, strat)
    check_accuracy(F, r, a, dtype)
    if kind == "kkt":
        assert r["last"][2] > 0
        check_solve(F, r, a, dtype, n)
    if kind == "spd":
        check_solve(F, r, a, dtype, n)
    if kind in ("identity", "zero"):
        assert r["count"] == 0 and not r["sub"].any() and np.array_equal(np.tril(r["packed"]), np.tril(a))


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_golden_exact(name, strat, dtype, it):
    F = init_gpu()
    case = GOLDEN["cases"][name]
    exp = case["expected"][strat]
    a = np.array(case["a"], dtype=dtype)
    n = a.shape[0]
    r = factor(F, a, strat, it)
    il = np.tril_indices(n)
    assert np.array_equal(r["packed"][il], np.array(exp["packed"], dtype=dtype)[il])
    assert np.array_equal(r["sub"], np.array(exp["subdiag"], dtype=dtype))
    assert list(r["pf"]) == exp["perm_fwd"] and r["count"] == exp["transposition_count"]
    assert r["last"][2] == exp["npiv"].count(2)


@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("n", sorted(int(k) for k in GOLDEN["parity_seeds"]))
def test_pivot_parity(n, strat):
    F = init_gpu()
    a = ref.random_symmetric(n, GOLDEN["parity_seeds"][str(n)]["seed"])
    e = ref.lblt_unblocked(a, strat)
    assert e["margin"] >= GOLDEN["margin"], e["margin"]  # rounding differences of a blocked fp64 run are ~1e-13
    r = factor(F, a, strat)
    assert np.array_equal(r["pf"].astype(np.int64), e["perm_fwd"]) and r["count"] == e["transposition_count"]
    assert np.array_equal(r["sub"] != 0, e["subdiag"] != 0)
    scale = max(np.abs(e["L"]).max(), 1.0)
    bound = 64 * n * EPS[np.dtype(np.float64)]
    assert np.abs(np.tril(r["packed"], -1) - np.tril(e["packed"], -1)).max(initial=0.0) <= bound * scale
    dscale = max(np.abs(e["d"]).max(), np.abs(e["subdiag"]).max())
    assert np.abs(np.diag(r["packed"]) - e["d"]).max() <= bound * scale * dscale
    assert np.abs(r["sub"] - e["subdiag"]).max() <= bound * scale * dscale


# ------------------------------------------------------------------------------------------------ views
def _strided_vec(n, step, dtype):
    import torch

    full = torch.from_numpy(np.full(step * n + 3, -3.25, dtype=dtype)).cuda()
    return full, full[1:1 + step * n:step]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["mat", "sub", "odd", "rowpad", "step2"])
@pytest.mark.parametrize("n", [40, 130])
def test_views(n, layout, dtype):
    F = init_gpu()
    a = np.asarray(ref.random_symmetric(n, 77 + n), dtype=dtype)
    base = factor(F, a, "partial_diag", nan_upper=False)
    box = view_box((n, n), layout, dtype)
    parent, v = place(a, layout)
    parent0 = parent.clone()
    sub_full, sub = _strided_vec(n, 2, dtype)
    _, pf, pb, cnt = F.lblt_factor_in_place(v, subdiag=sub)
    F.synchronize()
    guard_intact(parent, parent0, box, "lblt factor")
    il = np.tril_indices(n)
    assert np.array_equal(to_host(v)[il], base["packed"][il]) and np.array_equal(to_host(sub), base["sub"])
    assert np.array_equal(pf, base["pf"]) and cnt == base["count"]
    assert (to_host(sub_full)[0::2][: n + 1] == -3.25).all()
    # solve / reconstruct / inverse on the view, with a strided diag of its own and a placed right-hand side
    dg_full, dg = _strided_vec(n, 3, dtype)
    dg.copy_(v.diagonal())
    b = np.asarray(np.random.default_rng(n).standard_normal((n, 7)), dtype=dtype)
    xb = to_dev(np.array(b, order="F"))
    F.lblt_solve_in_place(base["dev"], base["sub_dev"], pf, pb, xb)
    bbox = view_box((n, 7), layout, dtype)
    xparent, xv = place(b, layout)
    xparent0 = xparent.clone()
    F.lblt_solve_in_place(v, sub, pf, pb, xv, diag=dg)
    F.synchronize()
    guard_intact(xparent, xparent0, bbox, "lblt solve")
    assert np.array_equal(to_host(xv), to_host(xb))
    for fn in (F.lblt_reconstruct, F.lblt_inverse):
        ref_out = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
        fn(ref_out, base["dev"], base["sub_dev"], pf, pb)
        oparent, ov = place(np.full((n, n), -7.5, dtype=dtype), layout)
        oparent0 = oparent.clone()
        fn(ov, v, sub, pf, pb, diag=dg)
        F.synchronize()
        guard_intact(oparent, oparent0, box, fn.__name__)
        assert np.array_equal(to_host(ov), to_host(ref_out))


@pytest.mark.parametrize("n", [40, 130])
def test_negative_strides(n):
    """A and rhs with their rows reversed in memory (negative row stride), through the C boundary"""
    import torch

    F = init_gpu()
    L = F.lib()
    a = ref.random_symmetric(n, 9 + n)
    base = factor(F, a, "partial_diag", nan_upper=False)
    t = to_dev(np.array(a[::-1], order="F"))  # logical (i, j) = stored (n - 1 - i, j)
    sub = torch.zeros(n, dtype=torch.float64, device="cuda")
    pf, pb = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    A = F.MatMut(t.data_ptr() + (n - 1) * 8, n, n, -1, n)
    p = L.libfaer_v0_23_LbltParams_f64()
    st = L.libfaer_v0_23_lblt_factor_in_place_u64_f64(A, F.VecMut(sub.data_ptr() + (n - 1) * 8, n, -1), F.SliceMut(pf.ctypes.data, n),
                                                     F.SliceMut(pb.ctypes.data, n), F.PAR_SEQ, F.MemAlloc(None, 0), p)
    assert st.tag == 0 and st.transposition_count == base["count"] and np.array_equal(pf, base["pf"])
    il = np.tril_indices(n)
    assert np.array_equal(to_host(t)[::-1][il], base["packed"][il])
    assert np.array_equal(to_host(sub)[::-1], base["sub"])
    b = np.random.default_rng(n).standard_normal((n, 3))
    xb = to_dev(np.array(b, order="F"))
    F.lblt_solve_in_place(base["dev"], base["sub_dev"], pf, pb, xb)
    x = to_dev(np.array(b[::-1], order="F"))
    dg = torch.zeros(n, dtype=torch.float64, device="cuda")
    dg.copy_(torch.from_numpy(np.ascontiguousarray(np.diag(base["packed"])[::-1])))
    L.libfaer_v0_23_lblt_solve_in_place_u64_f64(F.MatRef(t.data_ptr() + (n - 1) * 8, n, n, -1, n), F.VecRef(dg.data_ptr() + (n - 1) * 8, n, -1),
                                                F.VecRef(sub.data_ptr() + (n - 1) * 8, n, -1), C.c_int(0), F.SliceRef(pf.ctypes.data, n),
                                                F.SliceRef(pb.ctypes.data, n), F.MatMut(x.data_ptr() + (n - 1) * 8, n, 3, -1, n), F.PAR_SEQ,
                                                F.MemAlloc(None, 0))
    assert np.array_equal(to_host(x)[::-1], to_host(xb))


@pytest.mark.parametrize("n", [40, 130])
def test_host_operands(n):
    F = init_gpu()
    a = ref.random_symmetric(n, 31 + n)
    base = factor(F, a, "partial_diag", nan_upper=False)
    h = np.array(a, order="F")
    h[np.triu_indices(n, 1)] = np.nan
    sub = np.zeros(n)
    _, pf, pb, cnt = F.lblt_factor_in_place(h, subdiag=sub)
    il = np.tril_indices(n)
    assert np.array_equal(h[il], base["packed"][il]) and np.array_equal(sub, base["sub"]) and np.array_equal(pf, base["pf"])
    assert np.isnan(h[np.triu_indices(n, 1)]).all()
    b = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 7)))
    x = b.copy(order="F")
    F.lblt_solve_in_place(h, sub, pf, pb, x)
    assert np.linalg.norm(a @ x - b) <= tol(n, np.float64) * np.linalg.norm(a) * np.linalg.norm(x)
    out = np.full((n, n), -7.5, order="F")
    F.lblt_reconstruct(out, h, sub, pf, pb)
    assert (out[np.triu_indices(n, 1)] == -7.5).all() and np.abs(out[il] - a[il]).max() <= tol(n, np.float64) * np.abs(a).max()
