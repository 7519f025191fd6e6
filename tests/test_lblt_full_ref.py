"""CPU tests of tests/lblt_full_ref.py, the NumPy restatement of the Full pivoting strategy that the GPU tests compare with."""
import json
import os

import numpy as np
import pytest

import lblt_full_ref as fref
import lblt_ref as ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lblt_full_cases.json")))
SIZES = sorted(int(k) for k in GOLDEN["parity_seeds"])
EPS = np.finfo(np.float64).eps
_CACHE = {}


def matrix(kind, n):
    return ref.random_symmetric(n, 1000 + n) if kind == "gaussian" else ref.kkt(n, 7)


def factored(kind, n):
    if (kind, n) not in _CACHE:
        _CACHE[kind, n] = fref.lblt_full(matrix(kind, n))
    return _CACHE[kind, n]


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_golden(name):
    case = GOLDEN["cases"][name]
    exp = case["expected"]
    r = fref.lblt_full(np.array(case["a"]))
    assert np.array_equal(r["packed"], np.array(exp["packed"])) and np.array_equal(r["subdiag"], np.array(exp["subdiag"]))
    assert list(r["perm_fwd"]) == exp["perm_fwd"] and r["transposition_count"] == exp["transposition_count"]
    assert r["npiv"] == exp["npiv"] and r["tail_from"] == exp["tail_from"]
    for v in (exp["packed"], exp["subdiag"], case["a"]):  # every number survives float32
        assert np.array_equal(np.array(v, dtype=np.float32).astype(np.float64), np.array(v))


def test_golden_covers_the_named_properties():
    c = {k: v["expected"] for k, v in GOLDEN["cases"].items()}
    assert set(c) == {"pure_1x1", "zero_diagonal_2x2", "offdiag_tie_column_then_row", "diagonal_tie", "second_swap_moves_first",
                      "diagonal_unsorted", "blockdiag_early_exit", "zero"}
    assert c["pure_1x1"]["npiv"] == [1, 1, 1] and c["zero_diagonal_2x2"]["npiv"][0] == 2
    assert c["offdiag_tie_column_then_row"]["perm_fwd"][:2] == [0, 3] and c["diagonal_tie"]["perm_fwd"][0] == 1
    assert c["second_swap_moves_first"]["perm_fwd"][:2] == [1, 2] and c["diagonal_unsorted"]["tail_from"] == 0
    assert 0 < c["blockdiag_early_exit"]["tail_from"] < 5 and c["zero"]["transposition_count"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_parity_seed_margin(n):
    rec = GOLDEN["parity_seeds"][str(n)]
    assert fref.lblt_full(ref.random_symmetric(n, rec["seed"]))["margin"] >= GOLDEN["margin"]
    if rec["candidates_rejected"]:
        assert fref.lblt_full(ref.random_symmetric(n, rec["seed"] - 1))["margin"] < GOLDEN["margin"]


@pytest.mark.parametrize("kind", ["gaussian", "kkt"])
@pytest.mark.parametrize("n", SIZES)
def test_reconstruction(n, kind):
    a = matrix(kind, n)
    r = factored(kind, n)
    pf = r["perm_fwd"]
    assert sorted(pf) == list(range(n)) and np.array_equal(pf[r["perm_bwd"]], np.arange(n))
    res = np.abs(a[np.ix_(pf, pf)] - r["L"] @ ref.block_diag(r["d"], r["subdiag"]) @ r["L"].T).max()
    assert res <= 64 * n * EPS * np.abs(a).max()
    assert np.abs(ref.lblt_reconstruct(r["L"], r["d"], r["subdiag"], pf) - a).max() <= 64 * n * EPS * np.abs(a).max()
    if kind == "kkt" and n > 5:
        assert 2 in r["npiv"]
    assert sum(r["npiv"]) == n and np.count_nonzero(r["subdiag"]) == r["npiv"].count(2)


@pytest.mark.parametrize("k", [-40, -3, 5, 60])
@pytest.mark.parametrize("n", [5, 66])
def test_power_of_two_scaling(n, k):
    base = factored("gaussian", n)
    r = fref.lblt_full(matrix("gaussian", n) * 2.0 ** k)
    assert np.array_equal(r["L"], base["L"]) and np.array_equal(r["perm_fwd"], base["perm_fwd"]) and r["npiv"] == base["npiv"]
    assert np.array_equal(r["d"], base["d"] * 2.0 ** k) and np.array_equal(r["subdiag"], base["subdiag"] * 2.0 ** k)


@pytest.mark.parametrize("n", [5, 66])
def test_strict_upper_triangle_is_not_read(n):
    a = matrix("gaussian", n)
    b = a.copy()
    b[np.triu_indices(n, 1)] = np.nan
    r, s = factored("gaussian", n), fref.lblt_full(b)
    assert np.array_equal(r["packed"], s["packed"]) and np.array_equal(r["subdiag"], s["subdiag"])
    assert np.array_equal(r["perm_fwd"], s["perm_fwd"]) and r["margin"] == s["margin"]
