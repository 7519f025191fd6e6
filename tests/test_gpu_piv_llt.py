"""GPU tests of the Cholesky factorization with diagonal pivoting (include/faer_hip.h section 2h, csrc/piv_llt.hip) against
tests/piv_llt_ref.py."""
import json
import os

import numpy as np
import pytest

import piv_llt_ref as ref
from gpu_util import EPS, boosted, guard_intact, init_gpu, place, same_bits, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "piv_llt_cases.json")))
NB = 64  # panel width of csrc/piv_llt.hip
# the leaf alone, the first panel plus a leaf of 1 or 2 rows, two and three panels
SIZES = [1, 2, 3, 5, NB - 1, NB, NB + 1, NB + 2, 2 * NB + 1, 2 * NB + 2, 200]
DTYPES = [np.float64, np.float32]
ITYPES = [np.uint32, np.uint64]


def tol(n, dtype, c=64):
    """the bound tests/test_gpu_extras.py uses for the ldlt reconstruction"""
    return c * max(n, 1) * EPS[np.dtype(dtype)]


def factor(F, a, it=np.uint64, nan_upper=True):
    """factors the lower triangle of the numpy matrix `a` on the device; the strict upper triangle holds NaN on entry.  The status
    is returned, not raised."""
    import torch

    n = a.shape[0]
    a_in = np.array(a, order="F")
    if nan_upper:
        a_in[np.triu_indices(n, 1)] = np.nan
    d0 = to_dev(a_in)
    d = d0.clone()
    st = F.piv_llt_factor_in_place(d, index_dtype=it, raise_on_error=False)
    F.synchronize()
    last = F.debug_piv_llt_last()
    assert same_bits(torch.triu(d, 1), torch.triu(d0, 1)), "the strict upper triangle was written"
    r = {"dev": d, "dev0": d0, "packed": to_host(d), "last": last}
    if isinstance(st, tuple):
        r.update(ok=True, pf=st[0], pb=st[1], rank=st[2], count=st[3])
    else:
        r.update(ok=False, tag=st.tag, index=st.index)
    return r


def check_perm(r, n):
    pf, pb = r["pf"].astype(np.int64), r["pb"].astype(np.int64)
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[pb], np.arange(n))
    assert round(np.linalg.det(np.eye(n)[pf])) == (-1) ** r["count"]


def lower(r, rank=None):
    """L of the returned factorization in float64, its first `rank` columns"""
    L = np.tril(r["packed"].astype(np.float64))
    return L if rank is None else L[:, :rank]


def residual(r, a, rank=None):
    pf = r["pf"].astype(np.int64)
    L = lower(r, rank)
    return np.abs(np.asarray(a, dtype=np.float64)[np.ix_(pf, pf)] - L @ L.T).max()


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_spd(n, dtype, it):
    F = init_gpu()
    a = np.asarray(ref.spd(n, 1000 + n), dtype=dtype)
    a64 = a.astype(np.float64)
    r = factor(F, a, it)
    assert r["ok"] and r["rank"] == n and r["pf"].dtype == it
    check_perm(r, n)
    amax = np.abs(a64).max()
    print("residual", residual(r, a), "bound", tol(n, dtype) * amax)
    assert residual(r, a) <= tol(n, dtype) * amax
    panels, leaf_rows, cols, syncs = r["last"]
    assert (panels > 0) == (n > NB) and cols == n and syncs == 0 and 0 < leaf_rows <= NB
    il, iu = np.tril_indices(n), np.triu_indices(n, 1)
    # reconstruct: the lower triangle only
    out = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
    F.piv_llt_reconstruct(out, r["dev"], r["pf"], r["pb"])
    got = to_host(out)
    assert (got[iu] == -7.5).all()
    assert np.abs(got[il].astype(np.float64) - a64[il]).max() <= tol(n, dtype) * amax
    # solve
    for k in (1, 7):
        b = np.asarray(np.random.default_rng(n + k).standard_normal((n, k)), dtype=dtype, order="F")
        x = to_dev(b)
        F.piv_llt_solve_in_place(r["dev"], r["pf"], r["pb"], x)
        xs = to_host(x).astype(np.float64)
        assert np.linalg.norm(a64 @ xs - b) <= tol(n, dtype) * np.linalg.norm(a64) * np.linalg.norm(xs), (k,)
    # inverse: the lower triangle only, against the solve on the identity (symmetrised: A^-1 is symmetric)
    inv = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
    F.piv_llt_inverse(inv, r["dev"], r["pf"], r["pb"])
    eye = to_dev(np.eye(n, dtype=dtype))
    F.piv_llt_solve_in_place(r["dev"], r["pf"], r["pb"], eye)
    ginv, sinv = to_host(inv), to_host(eye).astype(np.float64)
    sinv = (sinv + sinv.T) / 2
    assert (ginv[iu] == -7.5).all()
    # two computed inverses: the forward error of each is of the order n eps cond(A) max |A^-1| (cond(A) ~ 5 for G G^T + n I)
    assert np.abs(ginv[il].astype(np.float64) - sinv[il]).max() <= tol(n, dtype) * np.abs(sinv).max() * np.linalg.cond(a64)
    # the content of the upper triangle does not matter
    plain = factor(F, a, it, nan_upper=False)
    assert np.array_equal(plain["packed"][il], r["packed"][il])
    assert np.array_equal(plain["pf"], r["pf"]) and plain["count"] == r["count"] and plain["rank"] == n


def embed(a, n):
    out = np.zeros((n, n))
    out[:a.shape[0], :a.shape[0]] = a
    return out


EXACT = [(name, None) for name in sorted(GOLDEN["cases"])] + [("diag_b_zero", NB + 2), ("diag_b_zero", 2 * NB + 2)]


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,size", EXACT)
def test_golden_exact(name, size, dtype, it):
    F = init_gpu()
    case = GOLDEN["cases"][name]
    exp = case["expected"]
    a = np.array(case["a"])
    L = np.array(exp["L"])
    pf = list(exp["perm_fwd"])
    if size is not None:  # the zero block grows: the factorization is the same, exactly, and stops inside the first panel
        pf = pf + list(range(a.shape[0], size))
        a, L = embed(a, size), embed(L, size)
    n, rank = a.shape[0], exp["rank"]
    r = factor(F, np.asarray(a, dtype=dtype), it)
    assert r["ok"] and r["rank"] == rank and r["count"] == exp["transposition_count"]
    assert list(r["pf"]) == pf
    check_perm(r, n)
    assert np.array_equal(np.tril(r["packed"])[:, :rank], L[:, :rank].astype(dtype))
    if rank < n:
        assert r["packed"][rank, rank] == 0
    panels, leaf_rows, cols, syncs = r["last"]
    assert cols == rank and syncs == 0 and (panels > 0) == (n > NB) and (leaf_rows == 0) == (n > NB and rank < n)


@pytest.mark.parametrize("n", sorted(int(k) for k in GOLDEN["full_rank_seeds"]))
def test_pivot_parity_full_rank(n):
    F = init_gpu()
    a = ref.spd(n, GOLDEN["full_rank_seeds"][str(n)]["seed"])
    e = ref.piv_llt_unblocked(a)
    assert e["status"] == "ok" and e["rank"] == n
    assert e["margin"] >= GOLDEN["margin"], e["margin"]  # rounding differences of a blocked fp64 run are ~1e-13
    r = factor(F, a)
    assert r["ok"] and r["rank"] == n
    assert np.array_equal(r["pf"].astype(np.int64), e["perm_fwd"]) and r["count"] == e["transposition_count"]
    scale = np.abs(e["L"]).max()
    err = np.abs(lower(r) - e["L"]).max()
    print("L error", err, "bound", tol(n, np.float64) * scale)
    assert err <= tol(n, np.float64) * scale


@pytest.mark.parametrize("n", sorted(int(k) for k in GOLDEN["low_rank_seeds"]))
def test_pivot_parity_low_rank(n):
    F = init_gpu()
    a = ref.low_rank(n, GOLDEN["low_rank_seeds"][str(n)]["seed"])
    e = ref.piv_llt_unblocked(a)
    rank = n // 2
    assert e["status"] == "ok" and e["rank"] == rank
    assert e["margin"] >= GOLDEN["margin"] and e["exit_ratio"] <= GOLDEN["exit_ratio"], (e["margin"], e["exit_ratio"])
    r = factor(F, a)
    assert r["ok"] and r["rank"] == rank, r
    check_perm(r, n)
    # the first `rank` pivots: the rows they brought to the front (the rest of the permutation is whatever they displaced)
    assert np.array_equal(r["pf"].astype(np.int64)[:rank], e["perm_fwd"][:rank])
    res = residual(r, a, rank)
    print("residual", res, "bound", tol(n, np.float64) * np.abs(a).max())
    assert res <= tol(n, np.float64) * np.abs(a).max()
    assert r["last"][2] == rank and r["last"][3] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, NB + 2])
def test_status(n, dtype):
    F = init_gpu()
    base = np.asarray(ref.spd(n, 7 + n), dtype=dtype)
    for bad in (-1.0, np.nan):  # a negative or NaN diagonal entry: NonPositivePivot{0}, A unmodified
        a = base.copy()
        a[n // 2, n // 2] = bad
        r = factor(F, a)
        assert not r["ok"] and r["tag"] == F.PIV_LLT_NON_POSITIVE_PIVOT and r["index"] == 0
        assert same_bits(r["dev"], r["dev0"])
        with pytest.raises(F.LltError) as ei:
            F.piv_llt_factor_in_place(to_dev(np.array(a, order="F")))
        assert ei.value.index == 0
    a = np.asarray(boosted(n), dtype=dtype)  # a NaN below the diagonal of the first pivot column reaches the diagonal at step 1
    a[n - 2, 0] = np.nan
    assert ref.piv_llt_unblocked(a)["index"] == 1
    r = factor(F, a)
    assert not r["ok"] and r["tag"] == F.PIV_LLT_NON_POSITIVE_PIVOT and r["index"] == 1
    r = factor(F, np.eye(n, dtype=dtype))
    assert r["ok"] and r["rank"] == n and r["count"] == 0 and np.array_equal(np.tril(r["packed"]), np.eye(n, dtype=dtype))
    assert list(r["pf"]) == list(range(n))
    # diag(I, 0): every arg-max is a tie, the stop falls in the last row (for n > NB: in the leaf that follows a panel)
    a = np.eye(n, dtype=dtype)
    a[n - 1, n - 1] = 0
    r = factor(F, a)
    assert r["ok"] and r["rank"] == n - 1 and r["count"] == 0 and np.array_equal(np.tril(r["packed"]), a)
    assert r["last"][1] == (n if n <= NB else n - NB)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_matrix(dtype):
    """the tolerance test is not made at step 0: 0 / sqrt(0) poisons step 1 for n >= 2, and order 1 is "rank 1" """
    F = init_gpu()
    r = factor(F, np.zeros((3, 3), dtype=dtype))
    assert not r["ok"] and r["tag"] == F.PIV_LLT_NON_POSITIVE_PIVOT and r["index"] == 1
    r = factor(F, np.zeros((1, 1), dtype=dtype))
    assert r["ok"] and r["rank"] == 1 and r["count"] == 0 and r["packed"][0, 0] == 0


# ------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["mat", "sub", "odd", "rowpad", "step2"])
@pytest.mark.parametrize("n", [40, 2 * NB + 2])
def test_views(n, layout, dtype):
    F = init_gpu()
    a = np.asarray(ref.spd(n, 77 + n), dtype=dtype)
    base = factor(F, a, nan_upper=False)
    box = view_box((n, n), layout, dtype)
    parent, v = place(a, layout)
    parent0 = parent.clone()
    pf, pb, rank, cnt = F.piv_llt_factor_in_place(v)
    F.synchronize()
    guard_intact(parent, parent0, box, "piv_llt factor")
    il = np.tril_indices(n)
    assert np.array_equal(to_host(v)[il], base["packed"][il])
    assert np.array_equal(pf, base["pf"]) and cnt == base["count"] and rank == n
    b = np.asarray(np.random.default_rng(n).standard_normal((n, 7)), dtype=dtype)
    xb = to_dev(np.array(b, order="F"))
    F.piv_llt_solve_in_place(base["dev"], pf, pb, xb)
    bbox = view_box((n, 7), layout, dtype)
    xparent, xv = place(b, layout)
    xparent0 = xparent.clone()
    F.piv_llt_solve_in_place(v, pf, pb, xv)
    F.synchronize()
    guard_intact(xparent, xparent0, bbox, "piv_llt solve")
    assert np.array_equal(to_host(xv), to_host(xb))
    for fn in (F.piv_llt_reconstruct, F.piv_llt_inverse):
        ref_out = to_dev(np.full((n, n), -7.5, dtype=dtype, order="F"))
        fn(ref_out, base["dev"], pf, pb)
        oparent, ov = place(np.full((n, n), -7.5, dtype=dtype), layout)
        oparent0 = oparent.clone()
        fn(ov, v, pf, pb)
        F.synchronize()
        guard_intact(oparent, oparent0, box, fn.__name__)
        assert np.array_equal(to_host(ov), to_host(ref_out))


@pytest.mark.parametrize("n", [40, 2 * NB + 2])
def test_negative_strides(n):
    """A and rhs with their rows reversed in memory (negative row stride), through the C boundary"""
    import ctypes as C

    F = init_gpu()
    L = F.lib()
    a = ref.spd(n, 9 + n)
    base = factor(F, a, nan_upper=False)
    t = to_dev(np.array(a[::-1], order="F"))  # logical (i, j) = stored (n - 1 - i, j)
    pf, pb = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    A = F.MatMut(t.data_ptr() + (n - 1) * 8, n, n, -1, n)
    p = L.libfaer_v0_23_PivLltParams_f64()
    st = L.libfaer_v0_23_piv_llt_factor_in_place_u64_f64(A, F.SliceMut(pf.ctypes.data, n), F.SliceMut(pb.ctypes.data, n), F.PAR_SEQ,
                                                        F.MemAlloc(None, 0), p)
    assert st.tag == 0 and st.rank == n and st.transposition_count == base["count"] and np.array_equal(pf, base["pf"])
    il = np.tril_indices(n)
    assert np.array_equal(to_host(t)[::-1][il], base["packed"][il])
    b = np.random.default_rng(n).standard_normal((n, 3))
    xb = to_dev(np.array(b, order="F"))
    F.piv_llt_solve_in_place(base["dev"], pf, pb, xb)
    x = to_dev(np.array(b[::-1], order="F"))
    L.libfaer_v0_23_piv_llt_solve_in_place_u64_f64(F.MatRef(t.data_ptr() + (n - 1) * 8, n, n, -1, n), F.SliceRef(pf.ctypes.data, n),
                                                   F.SliceRef(pb.ctypes.data, n), C.c_int(0), F.MatMut(x.data_ptr() + (n - 1) * 8, n, 3, -1, n),
                                                   F.PAR_SEQ, F.MemAlloc(None, 0))
    assert np.array_equal(to_host(x)[::-1], to_host(xb))


@pytest.mark.parametrize("n", [40, 2 * NB + 2])
def test_host_operands(n):
    F = init_gpu()
    a = ref.spd(n, 31 + n)
    base = factor(F, a, nan_upper=False)
    h = np.array(a, order="F")
    h[np.triu_indices(n, 1)] = np.nan
    pf, pb, rank, cnt = F.piv_llt_factor_in_place(h)
    il = np.tril_indices(n)
    assert np.array_equal(h[il], base["packed"][il]) and np.array_equal(pf, base["pf"]) and rank == n and cnt == base["count"]
    assert np.isnan(h[np.triu_indices(n, 1)]).all()
    b = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 7)))
    x = b.copy(order="F")
    F.piv_llt_solve_in_place(h, pf, pb, x)
    assert np.linalg.norm(a @ x - b) <= tol(n, np.float64) * np.linalg.norm(a) * np.linalg.norm(x)
    out = np.full((n, n), -7.5, order="F")
    F.piv_llt_reconstruct(out, h, pf, pb)
    assert (out[np.triu_indices(n, 1)] == -7.5).all() and np.abs(out[il] - a[il]).max() <= tol(n, np.float64) * np.abs(a).max()
