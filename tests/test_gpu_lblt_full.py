"""GPU tests of the Full pivoting strategy of the Bunch-Kaufman factorization (include/faer_hip.h section 2g, csrc/lblt.hip) against
tests/lblt_full_ref.py.  Tolerances, residual and the solve / reconstruct / inverse checks are those of tests/test_gpu_lblt.py."""
import json
import math
import os

import numpy as np
import pytest

import lblt_full_ref as fref
import lblt_ref as ref
from gpu_util import EPS, guard_intact, init_gpu, ordered_call, place, same_bits, same_result, to_dev, to_host, view_box
from test_gpu_lblt import check_accuracy, check_solve, residual, tol

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lblt_full_cases.json")))
SIZES = [1, 2, 3, 5, 63, 64, 65, 66, 129, 130, 200]
DTYPES = [np.float64, np.float32]
ITYPES = [np.uint32, np.uint64]
FULL = 4


def gpu():
    """the library, with the Full strategy: asserted before any factor call, so that a library without it fails here"""
    F = init_gpu()
    assert F.lblt_pivoting_supported(FULL) == 1
    return F


def factor(F, a, it=np.uint64, nan_upper=True):
    """factors the lower triangle of the numpy matrix `a` on the device with the Full strategy; the strict upper triangle holds NaN
    on entry (or the symmetric values) and must come back bit for bit"""
    import torch

    n = a.shape[0]
    a_in = np.array(a, order="F")
    if nan_upper:
        a_in[np.triu_indices(n, 1)] = np.nan
    d0 = to_dev(a_in)
    d = d0.clone()
    sub, pf, pb, cnt = F.lblt_factor_in_place(d, pivoting="full", index_dtype=it)
    F.synchronize()
    last = F.debug_lblt_last()
    assert same_bits(torch.triu(d, 1), torch.triu(d0, 1)), "the strict upper triangle was written"
    return {"dev": d, "sub_dev": sub, "packed": to_host(d), "sub": to_host(sub), "pf": pf, "pb": pb, "count": cnt, "last": last}


def check_structure(r, n):
    pf, pb = r["pf"].astype(np.int64), r["pb"].astype(np.int64)
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[pb], np.arange(n))
    assert round(np.linalg.det(np.eye(n)[pf])) == (-1) ** r["count"]
    sub, p = r["sub"], r["packed"]
    for j in range(n):
        if sub[j] != 0:
            assert j + 1 < n and sub[j + 1] == 0 and p[j + 1, j] == 0
    steps, leaf_rows, n2, syncs = r["last"]
    assert (leaf_rows == n) if n <= 64 else (leaf_rows in (63, 64))
    assert steps <= n - leaf_rows <= 2 * steps  # every step of the multi-workgroup path takes one or two rows
    assert n2 == np.count_nonzero(sub)
    assert syncs <= math.ceil(n / 64) + 1


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_gaussian(n, dtype, it):
    F = gpu()
    a = np.asarray(ref.random_symmetric(n, 1000 + n), dtype=dtype)
    r = factor(F, a, it)
    assert r["pf"].dtype == it
    check_structure(r, n)
    check_accuracy(F, r, a, dtype)
    check_solve(F, r, a, dtype, n)
    plain = factor(F, a, it, nan_upper=False)  # the content of the upper triangle does not matter
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
    if kind == "zero_row":
        a = ref.random_symmetric(n, 5)
        a[n // 2, :] = 0
        a[:, n // 2] = 0
        return a
    rng = np.random.default_rng(100 + n)
    if kind == "diagonal":  # unsorted, distinct magnitudes, both signs
        return np.diag(rng.permutation(np.arange(1.0, n + 1)) * rng.choice([-1.0, 1.0], n))
    assert kind == "blockdiag"  # a Gaussian block (40 rows, or 3 of 5) and a diagonal one: the main loop ends before the matrix does
    nb = min(40, n - 2)
    a = np.diag(rng.permutation(np.arange(1.0, n + 1)) / (1024.0 * n))  # (small: the main loop prefers the pivots of the Gaussian block)
    a[:nb, :nb] = ref.random_symmetric(nb, 9)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 66, 130])
@pytest.mark.parametrize("kind", ["kkt", "spd", "identity", "zero", "zero_row", "diagonal", "blockdiag"])
def test_special_inputs(kind, n, dtype):
    F = gpu()
    a = np.asarray(special(kind, n), dtype=dtype)
    r = factor(F, a)
    check_structure(r, n)
    check_accuracy(F, r, a, dtype)
    n2 = r["last"][2]
    if kind == "kkt":
        assert n2 > 0
        check_solve(F, r, a, dtype, n)
    if kind == "spd":
        assert n2 == 0
        check_solve(F, r, a, dtype, n)
    if kind in ("identity", "zero"):
        assert r["count"] == 0 and not r["sub"].any() and np.array_equal(np.tril(r["packed"]), np.tril(a))
    if kind == "diagonal":
        d = np.abs(np.diag(r["packed"]))
        assert n2 == 0 and (np.diff(d) < 0).all() and not np.tril(r["packed"], -1).any()
    if kind == "blockdiag":
        t0 = fref.lblt_full(a.astype(np.float64))["tail_from"]
        assert t0 < n and (n != 130 or t0 <= 60)  # the reference leaves its main loop early: at n = 130 before the leaf's rows begin
        t0 = min(t0 + 2, n)  # (two rows of slack for a 1 x 1 / 2 x 2 split that rounding decides differently)
        tail = np.abs(np.diag(r["packed"]))[t0:]
        assert (np.diff(tail) <= 0).all() and not np.tril(r["packed"], -1)[t0:, t0:].any()  # the tail orders what is left, across the hand-over


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_golden_exact(name, dtype, it):
    F = gpu()
    case = GOLDEN["cases"][name]
    exp = case["expected"]
    a = np.array(case["a"], dtype=dtype)
    n = a.shape[0]
    r = factor(F, a, it)
    il = np.tril_indices(n)
    assert np.array_equal(r["packed"][il], np.array(exp["packed"], dtype=dtype)[il])
    assert np.array_equal(r["sub"], np.array(exp["subdiag"], dtype=dtype))
    assert list(r["pf"]) == exp["perm_fwd"] and r["count"] == exp["transposition_count"]
    assert r["last"][2] == exp["npiv"].count(2)


@pytest.mark.parametrize("n", sorted(int(k) for k in GOLDEN["parity_seeds"]))
def test_pivot_parity(n):
    F = gpu()
    a = ref.random_symmetric(n, GOLDEN["parity_seeds"][str(n)]["seed"])
    e = fref.lblt_full(a)
    assert e["margin"] >= GOLDEN["margin"], e["margin"]
    r = factor(F, a)
    assert np.array_equal(r["pf"].astype(np.int64), e["perm_fwd"]) and r["count"] == e["transposition_count"]
    assert np.array_equal(r["sub"] != 0, e["subdiag"] != 0)
    scale = max(np.abs(e["L"]).max(), 1.0)
    bound = 64 * n * EPS[np.dtype(np.float64)]
    assert np.abs(np.tril(r["packed"], -1) - np.tril(e["packed"], -1)).max(initial=0.0) <= bound * scale
    dscale = max(np.abs(e["d"]).max(), np.abs(e["subdiag"]).max())
    assert np.abs(np.diag(r["packed"]) - e["d"]).max() <= bound * scale * dscale
    assert np.abs(r["sub"] - e["subdiag"]).max() <= bound * scale * dscale


# ------------------------------------------------------------------------------------------------ views and hosts
def _strided_vec(n, step, dtype):
    import torch

    full = torch.from_numpy(np.full(step * n + 3, -3.25, dtype=dtype)).cuda()
    return full, full[1:1 + step * n:step]


@pytest.mark.parametrize("layout", ["mat", "sub"])  # a padded and an offset device view
def test_views(layout):
    F = gpu()
    n, dtype = 130, np.float64
    a = ref.random_symmetric(n, 77 + n)
    base = factor(F, a, nan_upper=False)
    box = view_box((n, n), layout, dtype)
    parent, v = place(a, layout)
    parent0 = parent.clone()
    _, pf, pb, cnt = F.lblt_factor_in_place(v, pivoting="full")
    F.synchronize()
    guard_intact(parent, parent0, box, "lblt full factor")
    il = np.tril_indices(n)
    assert np.array_equal(to_host(v)[il], base["packed"][il]) and np.array_equal(pf, base["pf"]) and cnt == base["count"]


def test_strided_subdiag():
    F = gpu()
    n = 130
    a = ref.random_symmetric(n, 78 + n)
    base = factor(F, a, nan_upper=False)
    sub_full, sub = _strided_vec(n, 2, np.float64)
    d = to_dev(np.array(a, order="F"))
    _, pf, _, cnt = F.lblt_factor_in_place(d, subdiag=sub, pivoting="full")
    il = np.tril_indices(n)
    assert np.array_equal(to_host(d)[il], base["packed"][il]) and np.array_equal(to_host(sub), base["sub"])
    assert np.array_equal(pf, base["pf"]) and cnt == base["count"]
    assert (to_host(sub_full)[0::2][: n + 1] == -3.25).all()


def test_host_operands():
    F = gpu()
    n = 130
    a = ref.random_symmetric(n, 31 + n)
    base = factor(F, a, nan_upper=False)
    h = np.array(a, order="F")
    h[np.triu_indices(n, 1)] = np.nan
    sub = np.zeros(n)
    _, pf, pb, cnt = F.lblt_factor_in_place(h, subdiag=sub, pivoting=FULL)
    il = np.tril_indices(n)
    assert np.array_equal(h[il], base["packed"][il]) and np.array_equal(sub, base["sub"]) and np.array_equal(pf, base["pf"])
    assert np.isnan(h[np.triu_indices(n, 1)]).all() and cnt == base["count"]
    b = np.asfortranarray(np.random.default_rng(n).standard_normal((n, 7)))
    x = b.copy(order="F")
    F.lblt_solve_in_place(h, sub, pf, pb, x)
    assert np.linalg.norm(a @ x - b) <= tol(n, np.float64) * np.linalg.norm(a) * np.linalg.norm(x)


def test_owner():
    F = gpu()
    n = 66
    a = ref.random_symmetric(n, 5 + n)
    o = F.Lblt(to_dev(a), pivoting="full")
    assert F.debug_lblt_last()[1] in (63, 64) and np.abs(to_host(o.reconstruct())[np.tril_indices(n)] - a[np.tril_indices(n)]).max() <= tol(n, np.float64) * np.abs(a).max()
    b = np.random.default_rng(n).standard_normal((n, 3))
    x = to_host(o.solve_in_place(to_dev(b)))
    assert np.linalg.norm(a @ x - b) <= tol(n, np.float64) * np.linalg.norm(a) * np.linalg.norm(x)


# ------------------------------------------------------------------------------------------------ poisoned scratch
def test_poisoned_scratch():
    """every scratch buffer of the call filled with 0xFF / 0x7F bytes before use: the same bits as without the fill"""
    F = gpu()
    n = 130
    a = ref.random_symmetric(n, 1000 + n)

    def run():
        r = factor(F, a)
        return {k: r[k] for k in ("packed", "sub", "pf", "pb", "count")}

    try:
        F.debug_scratch_fill(-1)
        base = run()
        outs = []
        for byte in (0xFF, 0x7F):
            F.debug_scratch_fill(byte)
            outs.append(run())
            F.synchronize()
            count, nbytes = F.debug_scratch_fill_stats()
            assert count > 0 and nbytes >= 256 * count, (byte, count, nbytes)
    finally:
        F.debug_scratch_fill(-1)
    assert residual({**base}, a) <= tol(n, np.float64) * np.abs(a).max()
    for o in outs:
        il = np.tril_indices(n)
        same_result({**base, "packed": base["packed"][il]}, {**o, "packed": o["packed"][il]}, "lblt full, poisoned scratch")


# ------------------------------------------------------------------------------------------------ caller stream
def test_caller_stream():
    """between a producer and a consumer queued on a non-blocking stream, with no host synchronisation around the call"""
    F = gpu()
    n = 130
    good = {"a": ref.random_symmetric(n, 1006), "sub": np.full((n, 1), -7.5)}
    stale = {"a": ref.random_symmetric(n, 2006), "sub": np.full((n, 1), -3.25)}

    def call(b):
        _, pf, pb, cnt = F.lblt_factor_in_place(b["a"], subdiag=b["sub"][:, 0], pivoting="full")
        return {"lb": b["a"], "sub": b["sub"], "pf": pf, "pb": pb, "count": cnt}

    expected, got = ordered_call(call, good, stale)
    same_result(expected, got, "lblt full on a caller stream")
    pf = expected["pf"].astype(np.int64)
    L = ref.unit_lower(expected["lb"])
    res = np.abs(good["a"][np.ix_(pf, pf)] - L @ ref.block_diag(np.diag(expected["lb"]), expected["sub"][:, 0]) @ L.T).max()
    assert res <= tol(n, np.float64) * np.abs(good["a"]).max()
