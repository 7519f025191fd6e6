"""CPU tests of tests/lblt_ref.py, the NumPy restatement the GPU tests of the Bunch-Kaufman factorization compare against."""
import json
import math
import os

import numpy as np
import pytest

import lblt_ref as ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lblt_cases.json")))
EPS = np.finfo(np.float64).eps
STRATS = list(ref.STRATEGIES)


@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_golden_cases_exact(name, strat):
    case = GOLDEN["cases"][name]
    exp = case["expected"][strat]
    r = ref.lblt_unblocked(np.array(case["a"]), strat)
    assert np.array_equal(r["packed"], np.array(exp["packed"]))
    assert np.array_equal(r["subdiag"], np.array(exp["subdiag"]))
    assert list(r["perm_fwd"]) == exp["perm_fwd"] and r["transposition_count"] == exp["transposition_count"]
    assert r["npiv"] == exp["npiv"]
    # hand check: P A P^T == L B L^T exactly, and the solve inverts it
    a = np.array(case["a"])
    pf = r["perm_fwd"]
    assert np.array_equal(a[np.ix_(pf, pf)], r["L"] @ ref.block_diag(r["d"], r["subdiag"]) @ r["L"].T)
    assert np.array_equal(ref.lblt_reconstruct(r["L"], r["d"], r["subdiag"], pf), a)


def test_golden_coverage():
    c = GOLDEN["cases"]
    assert all(v == 1 for v in c["pure_1x1"]["expected"]["partial"]["npiv"])
    assert 2 in c["zero_diagonal_2x2"]["expected"]["partial"]["npiv"] and not np.diag(np.array(c["zero_diagonal_2x2"]["a"])).any()
    a = np.array(c["tie_lowest_index"]["a"])
    assert abs(a[1, 0]) == abs(a[2, 0]) and c["tie_lowest_index"]["expected"]["partial"]["perm_fwd"] == [0, 1, 2]
    assert not np.array(c["zero_column"]["a"])[:, 0].any()
    assert c["partial_vs_rook"]["expected"]["partial"]["perm_fwd"] != c["partial_vs_rook"]["expected"]["rook"]["perm_fwd"]


@pytest.mark.parametrize("strat", STRATS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 64, 65, 130])
def test_random_residual_structure_and_growth(n, strat):
    a = ref.random_symmetric(n, 100 + n)
    r = ref.lblt_unblocked(a, strat)
    pf, pb = r["perm_fwd"], r["perm_bwd"]
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[pb], np.arange(n))
    res = a[np.ix_(pf, pf)] - r["L"] @ ref.block_diag(r["d"], r["subdiag"]) @ r["L"].T
    assert np.abs(res).max() <= 64 * n * EPS * np.abs(a).max()
    assert sum(r["npiv"]) == n
    for j in range(n - 1):
        if r["subdiag"][j] != 0:
            assert r["subdiag"][j + 1] == 0 and r["packed"][j + 1, j] == 0
    if ref.STRATEGIES[strat][1]:  # rook: bounded multipliers
        assert np.abs(np.tril(r["L"], -1)).max(initial=0.0) <= 1.0 / (1.0 - ref.ALPHA) + 8 * n * EPS
    sign = round(np.linalg.det(np.eye(n)[pf]))
    assert sign == (-1) ** r["transposition_count"]
    b = np.random.default_rng(n).standard_normal((n, 3))
    x = ref.lblt_solve(r["L"], r["d"], r["subdiag"], pf, b)
    assert np.abs(a @ x - b).max() <= 64 * n * EPS * max(np.abs(a).max() * np.abs(x).max(), 1.0) * n


@pytest.mark.parametrize("strat", STRATS)
def test_parity_seeds_have_margin(strat):
    assert GOLDEN["margin"] == 1e-6
    for n, rec in GOLDEN["parity_seeds"].items():
        m = ref.lblt_unblocked(ref.random_symmetric(int(n), rec["seed"]), strat)["margin"]
        assert m >= GOLDEN["margin"] and math.isfinite(m), (n, m)


def test_kkt_has_2x2_pivots():
    r = ref.lblt_unblocked(ref.kkt(40, 3), "partial_diag")
    assert 2 in r["npiv"] and np.count_nonzero(r["subdiag"]) == r["npiv"].count(2)
