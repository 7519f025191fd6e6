"""Writes lblt_cases.json: hand-checkable exact cases of the Bunch-Kaufman factorization and the seeds of the pivot-parity tests.

Exact cases: small integer symmetric matrices whose whole elimination is exact in binary floating point (pivots that are powers of
two, 2 x 2 blocks whose determinant is minus a power of two), so every correct implementation must reproduce L, B, the permutation
and the transposition count bit for bit, in fp32 as in fp64.  The expected values come from tests/lblt_ref.py; this script accepts
them only if P A P^T == L B L^T holds EXACTLY and every number is a small dyadic rational.  They cover a pure 1 x 1 run, a zero
diagonal that forces 2 x 2 pivots, an arg-max tie (resolved to the lowest index), a zero column (gamma == 0) and a matrix on which
Partial and Rook choose different pivots.

Seeds: for every size of the parity test the first seed of tests/lblt_ref.random_symmetric whose minimum relative decision margin is
at least 1e-6 under all four strategies, with the number of candidates tried and rejected.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lblt_ref as ref  # noqa: E402

MATRICES = {
    "pure_1x1": [[4, 2, -2], [2, 3, 1], [-2, 1, 2]],
    "zero_diagonal_2x2": [[0, 1, 2, 0], [1, 0, 1, 0], [2, 1, 0, 2], [0, 0, 2, 0]],
    "tie_lowest_index": [[0, 2, 2], [2, 0, 1], [2, 1, 0]],
    "zero_column": [[0, 0, 0], [0, 2, 1], [0, 1, 1]],
    "partial_vs_rook": [[0, 1, 0, 0], [1, 0, 2, 0], [0, 2, 0, 1], [0, 0, 1, 0]],
}
PARITY_SIZES = [5, 63, 64, 65, 66, 129, 130, 200]
MARGIN = 1e-6


def dyadic(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x * 256 == np.round(x * 256)) and np.all(np.abs(x) < 256) and np.all(x.astype(np.float32) == x))


cases = {}
for name, rows in MATRICES.items():
    A = np.array(rows, dtype=np.float64)
    assert np.array_equal(A, A.T)
    per = {}
    for strat in ref.STRATEGIES:
        r = ref.lblt_unblocked(A, strat)
        B = ref.block_diag(r["d"], r["subdiag"])
        pf = r["perm_fwd"]
        assert np.array_equal(A[np.ix_(pf, pf)], r["L"] @ B @ r["L"].T), (name, strat)
        assert dyadic(r["L"]) and dyadic(B), (name, strat)
        per[strat] = {"packed": r["packed"].tolist(), "subdiag": r["subdiag"].tolist(), "perm_fwd": [int(v) for v in pf],
                      "transposition_count": int(r["transposition_count"]), "npiv": r["npiv"]}
    cases[name] = {"a": A.tolist(), "expected": per}
assert all(v == 1 for v in cases["pure_1x1"]["expected"]["partial"]["npiv"])
assert 2 in cases["zero_diagonal_2x2"]["expected"]["partial"]["npiv"]
assert cases["tie_lowest_index"]["expected"]["partial"]["perm_fwd"] == [0, 1, 2]
assert cases["partial_vs_rook"]["expected"]["partial"]["perm_fwd"] != cases["partial_vs_rook"]["expected"]["rook"]["perm_fwd"]

seeds = {}
for n in PARITY_SIZES:
    tried = 0
    for seed in range(100):
        tried += 1
        if all(ref.lblt_unblocked(ref.random_symmetric(n, seed), s)["margin"] >= MARGIN for s in ref.STRATEGIES):
            seeds[str(n)] = {"seed": seed, "candidates_rejected": tried - 1}
            break
    else:
        raise SystemExit(f"no seed with margin >= {MARGIN} at n = {n}")
out = {"source": "exact Bunch-Kaufman cases and parity seeds; expected values from tests/lblt_ref.py, verified exactly",
       "margin": MARGIN, "cases": cases, "parity_seeds": seeds}
with open(os.path.join(HERE, "lblt_cases.json"), "w") as f:
    json.dump(out, f, indent=1)
print({k: v for k, v in seeds.items()})
