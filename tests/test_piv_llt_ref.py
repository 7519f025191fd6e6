"""CPU tests of tests/piv_llt_ref.py, the NumPy restatement the GPU tests of the pivoted Cholesky factorization compare against."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import piv_llt_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "piv_llt_cases.json")))
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 64, 65, 130])
def test_spd_residual_and_structure(n):
    a = ref.spd(n, 100 + n)
    r = ref.piv_llt_unblocked(a)
    assert r["status"] == "ok" and r["rank"] == n and r["exit_ratio"] is None
    pf, pb = r["perm_fwd"], r["perm_bwd"]
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[pb], np.arange(n))
    assert np.abs(a[np.ix_(pf, pf)] - r["L"] @ r["L"].T).max() <= 64 * n * EPS * np.abs(a).max()
    assert round(np.linalg.det(np.eye(n)[pf])) == (-1) ** r["transposition_count"]
    d = np.diag(r["L"])
    assert np.all(d[:-1] >= d[1:]) and np.all(d > 0)  # the pivots of a pivoted Cholesky factorization do not increase
    assert np.abs(ref.piv_llt_reconstruct(r["L"], pf) - a).max() <= 64 * n * EPS * np.abs(a).max()
    b = np.random.default_rng(n).standard_normal((n, 3))
    x = ref.piv_llt_solve(r["L"], pf, b)
    assert np.linalg.norm(a @ x - b) <= 64 * n * EPS * np.linalg.norm(a) * np.linalg.norm(x)


def test_upper_triangle_is_not_read():
    a = ref.spd(9, 1)
    b = a.copy()
    b[np.triu_indices(9, 1)] = np.nan
    r, s = ref.piv_llt_unblocked(a), ref.piv_llt_unblocked(b)
    assert np.array_equal(r["L"], s["L"]) and np.array_equal(r["perm_fwd"], s["perm_fwd"])


def test_ties_go_to_the_lowest_index():
    r = ref.piv_llt_unblocked(np.eye(6))
    assert list(r["perm_fwd"]) == list(range(6)) and r["transposition_count"] == 0 and r["margin"] == 0
    assert np.array_equal(r["L"], np.eye(6))
    r = ref.piv_llt_unblocked(np.diag([1.0, 4.0, 4.0, 1.0]))
    assert list(r["perm_fwd"]) == [1, 2, 0, 3] and r["transposition_count"] == 2


def test_zero_matrix_outcomes():
    r = ref.piv_llt_unblocked(np.zeros((3, 3)))
    assert r["status"] == "non_positive_pivot" and r["index"] == 1
    r = ref.piv_llt_unblocked(np.zeros((1, 1)))
    assert r["status"] == "ok" and r["rank"] == 1 and r["transposition_count"] == 0
    assert ref.piv_llt_unblocked(np.zeros((0, 0)))["rank"] == 0


@pytest.mark.parametrize("bad", [-1.0, math.nan])
def test_negative_or_nan_diagonal(bad):
    a = ref.spd(5, 2)
    a[3, 3] = bad
    r = ref.piv_llt_unblocked(a)
    assert r["status"] == "non_positive_pivot" and r["index"] == 0
    assert np.array_equal(r["packed"][np.tril_indices(5)], a[np.tril_indices(5)], equal_nan=True)


def test_nan_below_the_diagonal():
    a = ref.spd(5, 2)
    a[0, 0] = 2 * np.diag(a).max()
    a[3, 0] = math.nan
    r = ref.piv_llt_unblocked(a)
    assert r["status"] == "non_positive_pivot" and r["index"] == 1


@pytest.mark.parametrize("k,z", [(1, 1), (4, 3), (7, 60)])
def test_rank_of_block_diagonal_inputs(k, z):
    a = np.zeros((k + z, k + z))
    a[:k, :k] = ref.spd(k, 5)
    r = ref.piv_llt_unblocked(a)
    assert r["status"] == "ok" and r["rank"] == k and r["exit_ratio"] == 0 and r["packed"][k, k] == 0
    assert sorted(r["perm_fwd"][:k]) == list(range(k))
    L = r["L"][:, :k]
    pf = r["perm_fwd"]
    assert np.abs(a[np.ix_(pf, pf)] - L @ L.T).max() <= 64 * (k + z) * EPS * np.abs(a).max()


@pytest.mark.parametrize("n", [5, 64, 130])
def test_low_rank(n):
    a = ref.low_rank(n, 3)
    r = ref.piv_llt_unblocked(a)
    assert r["status"] == "ok" and r["rank"] == n // 2 and 0 <= r["exit_ratio"] < 1
    L = r["L"][:, :r["rank"]]
    pf = r["perm_fwd"]
    assert sorted(pf) == list(range(n))
    assert np.abs(a[np.ix_(pf, pf)] - L @ L.T).max() <= 64 * n * EPS * np.abs(a).max()


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_golden_cases_exact(name):
    case = GOLDEN["cases"][name]
    exp = case["expected"]
    a = np.array(case["a"])
    r = ref.piv_llt_unblocked(a)
    assert np.array_equal(r["L"], np.array(exp["L"])) and list(r["perm_fwd"]) == exp["perm_fwd"]
    assert r["rank"] == exp["rank"] and r["transposition_count"] == exp["transposition_count"]
    pf = r["perm_fwd"]
    assert np.array_equal(a[np.ix_(pf, pf)], r["L"] @ r["L"].T)
    a32 = a.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), a) and np.array_equal(np.array(exp["L"]).astype(np.float32).astype(np.float64), exp["L"])


def test_parity_seeds_have_margin():
    assert GOLDEN["margin"] == 1e-6 and GOLDEN["exit_ratio"] == 0.125
    assert sorted(int(k) for k in GOLDEN["low_rank_seeds"]) == [5, 64, 66, 130, 200]
    for n, rec in GOLDEN["full_rank_seeds"].items():
        r = ref.piv_llt_unblocked(ref.spd(int(n), rec["seed"]))
        assert r["rank"] == int(n) and r["margin"] >= GOLDEN["margin"], (n, r["margin"])
    for n, rec in GOLDEN["low_rank_seeds"].items():
        r = ref.piv_llt_unblocked(ref.low_rank(int(n), rec["seed"]))
        assert r["rank"] == int(n) // 2 and r["margin"] >= GOLDEN["margin"] and r["exit_ratio"] <= GOLDEN["exit_ratio"], (n, r)


def test_golden_file_is_up_to_date(tmp_path):
    """a fresh run of the generator reproduces the committed file byte for byte"""
    spec = importlib.util.spec_from_file_location("make_piv_llt_cases", os.path.join(HERE, "golden", "make_piv_llt_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.main(str(tmp_path / "out.json"))
    assert open(tmp_path / "out.json", "rb").read() == open(os.path.join(HERE, "golden", "piv_llt_cases.json"), "rb").read()
