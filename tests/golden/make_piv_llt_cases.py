"""Writes piv_llt_cases.json: exact cases of the Cholesky factorization with diagonal pivoting and the seeds of the pivot-parity tests.

(a) Exact cases: matrices whose whole factorization is exact in binary floating point (every pivot a power of 4, every other number
a small dyadic rational), so every correct implementation must reproduce L, the permutation, the rank and the transposition count bit
for bit, in fp32 as in fp64.  The expected values come from tests/piv_llt_ref.py; this script accepts them only if P A P^T == L L^T
holds EXACTLY and every number is a small dyadic rational.  They cover a diagonal matrix in scrambled order, a product L L^T whose
rows pivoting has to reorder, arg-max ties (resolved to the lowest index) and diag(B, 0): an exact positive definite block followed by
a zero block, where the factorization stops with rank = dim B on trailing diagonals that are exactly 0.

(b) Full-rank parity seeds: for every size the first seed of piv_llt_ref.spd (G G^T + n I) whose minimum relative decision margin is
at least 1e-6, with the number of seeds rejected.

(c) Low-rank parity seeds: for every size of a fixed list the first seed of piv_llt_ref.low_rank (G G^T, G n x floor(n / 2)) with
that margin, rank floor(n / 2) and an exit pivot of at most tol / 8.

The script fails rather than widens if a size has no such seed within 100 tries.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import piv_llt_ref as ref  # noqa: E402

NB = 64  # panel width of csrc/piv_llt.hip: the full-rank sizes sit around its multiples
FULL_RANK_SIZES = [1, 2, 3, 5, NB - 1, NB, NB + 1, NB + 2, 2 * NB + 1, 2 * NB + 2, 200]
LOW_RANK_SIZES = [5, 64, 66, 130, 200]
MARGIN = 1e-6
EXIT_RATIO = 1.0 / 8

# the factor the pivoted run has to find: at every step its diagonal entry squared is the strict maximum of what is left
L_REORDER = np.array([[8, 0, 0, 0], [4, 4, 0, 0], [-2, 2, 2, 0], [1, -1, 1, 1]], dtype=np.float64)
SCRAMBLE = [2, 0, 3, 1]


def reorder_matrix():
    m = L_REORDER @ L_REORDER.T
    a = np.zeros_like(m)
    a[np.ix_(SCRAMBLE, SCRAMBLE)] = m
    return a


def diag_b_zero():
    a = np.zeros((7, 7))
    a[:4, :4] = reorder_matrix()
    return a


MATRICES = {
    "diagonal_powers_of_4": np.diag([4.0, 64.0, 1.0, 256.0, 16.0]),
    "reorder": reorder_matrix(),
    "tie_lowest_index": np.array([[16, 0, 4, 0], [0, 16, 0, 0], [4, 0, 5, 0], [0, 0, 0, 4]], dtype=np.float64),
    "diag_b_zero": diag_b_zero(),
}


def dyadic(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x * 256 == np.round(x * 256)) and np.all(np.abs(x) < 1024) and np.all(x.astype(np.float32) == x))


def main(dst=None):
    """writes the file next to this script, or to `dst` (tests: generate to a temporary file and compare)"""
    cases = {}
    for name, A in MATRICES.items():
        assert np.array_equal(A, A.T)
        r = ref.piv_llt_unblocked(A)
        assert r["status"] == "ok", name
        pf, rank, L = r["perm_fwd"], r["rank"], r["L"]
        assert np.array_equal(A[np.ix_(pf, pf)], L @ L.T), name
        assert dyadic(L) and dyadic(A), name
        cases[name] = {"a": A.tolist(), "expected": {"L": L.tolist(), "perm_fwd": [int(v) for v in pf], "rank": int(rank),
                                                     "transposition_count": int(r["transposition_count"])}}
    e = {k: v["expected"] for k, v in cases.items()}
    assert e["diagonal_powers_of_4"]["perm_fwd"] == [3, 1, 4, 0, 2] and e["diagonal_powers_of_4"]["rank"] == 5
    assert e["reorder"]["perm_fwd"] == SCRAMBLE and e["reorder"]["transposition_count"] > 0
    assert np.array_equal(np.array(e["reorder"]["L"]), L_REORDER)
    assert e["tie_lowest_index"]["perm_fwd"] == [0, 1, 2, 3] and e["tie_lowest_index"]["transposition_count"] == 0
    assert e["diag_b_zero"]["rank"] == 4 and e["diag_b_zero"]["perm_fwd"][:4] == SCRAMBLE

    full = {}
    for n in FULL_RANK_SIZES:
        for seed in range(100):
            r = ref.piv_llt_unblocked(ref.spd(n, seed))
            if r["status"] == "ok" and r["rank"] == n and r["margin"] >= MARGIN:
                full[str(n)] = {"seed": seed, "candidates_rejected": seed}
                break
        else:
            raise SystemExit(f"no full-rank seed with margin >= {MARGIN} at n = {n}")
    low = {}
    for n in LOW_RANK_SIZES:
        for seed in range(100):
            r = ref.piv_llt_unblocked(ref.low_rank(n, seed))
            if r["status"] == "ok" and r["rank"] == n // 2 and r["margin"] >= MARGIN and r["exit_ratio"] <= EXIT_RATIO:
                low[str(n)] = {"seed": seed, "candidates_rejected": seed}
                break
        else:
            raise SystemExit(f"no low-rank seed with margin >= {MARGIN} and exit pivot <= tol / 8 at n = {n}")
    out = {"source": "exact cases of the pivoted Cholesky factorization and parity seeds; expected values from tests/piv_llt_ref.py, "
                     "verified exactly",
           "margin": MARGIN, "exit_ratio": EXIT_RATIO, "cases": cases, "full_rank_seeds": full, "low_rank_seeds": low}
    with open(dst or os.path.join(HERE, "piv_llt_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
    return full, low


if __name__ == "__main__":
    print(main(*sys.argv[1:2]))
