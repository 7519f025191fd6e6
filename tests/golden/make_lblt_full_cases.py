"""Writes lblt_full_cases.json: exact cases of the Full pivoting strategy of the Bunch-Kaufman factorization and the seeds of its
pivot-parity test.

Exact cases: small symmetric integer matrices whose largest magnitude is a power of two, so that the scaling of the algorithm is
exact, and whose whole elimination is dyadic.  The expected values come from tests/lblt_full_ref.py; this script accepts a case only
if P A P^T == L B L^T holds EXACTLY, every number is a small dyadic rational that survives a round trip through float32, and the
case shows the property it is named after (asserted below).  Where a matrix has free entries (None in its template) the first
filling from {0, 1, -1}, in itertools.product order, that is accepted is taken.

Seeds: for every size of the parity test the first seed of tests/lblt_ref.random_symmetric whose minimum relative decision margin
under the Full strategy is at least 1e-6, with the number of candidates rejected.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lblt_full_ref as fref  # noqa: E402
import lblt_ref as ref  # noqa: E402

PARITY_SIZES = [5, 63, 64, 65, 66, 129, 130, 200]
MARGIN = 1e-6
N_ = None  # a free entry of a template (lower triangle; the upper one is mirrored)


def dyadic(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x * 256 == np.round(x * 256)) and np.all(np.abs(x) < 256) and np.all(x.astype(np.float32) == x))


def exact(A):
    """the reference's result if the case is exact, else None"""
    amax = np.abs(np.tril(A)).max()
    if amax != 0 and np.log2(amax) != np.round(np.log2(amax)):
        return None
    with np.errstate(all="ignore"):
        r = fref.lblt_full(A)
    B = ref.block_diag(r["d"], r["subdiag"])
    pf = r["perm_fwd"]
    if not (np.all(np.isfinite(r["L"])) and np.all(np.isfinite(B))):
        return None
    if not (np.array_equal(A[np.ix_(pf, pf)], r["L"] @ B @ r["L"].T) and dyadic(r["L"]) and dyadic(B) and dyadic(A)):
        return None
    return r


def first_offdiag(A):
    """(row, column) of the first largest |a| of the strict lower triangle in column-major order, and how often that value occurs"""
    n = A.shape[0]
    best, where, count = 0.0, None, 0
    for j in range(n):
        for i in range(j + 1, n):
            v = abs(A[i, j])
            if v > best:
                best, where, count = v, (i, j), 1
            elif v == best and best > 0:
                count += 1
    return where, count


def fill(template, accept):
    """the first filling of the free entries that is exact and accepted"""
    t = np.array([[np.nan if v is None else v for v in row] for row in template], dtype=np.float64)
    free = [(i, j) for i in range(t.shape[0]) for j in range(i + 1) if np.isnan(t[i, j])]
    for vals in itertools.product((0.0, 1.0, -1.0), repeat=len(free)):
        A = np.tril(t)
        for (i, j), v in zip(free, vals):
            A[i, j] = v
        A = np.tril(A) + np.tril(A, -1).T
        r = exact(A)
        if r is not None and accept(A, r):
            return A, r
    raise SystemExit("no exact filling of a template")


D4 = np.diag([1.0, -4.0, 2.0, 0.0, -2.0])
P3 = np.array([[4.0, 2, -2], [2, 3, 1], [-2, 1, 2]])
TEMPLATES = {
    # every step a 1 x 1 pivot of the main loop
    "pure_1x1": (P3.tolist(), lambda A, r: r["npiv"] == [1, 1, 1] and r["tail_from"] == 2),
    # a zero diagonal: 2 x 2 pivots
    "zero_diagonal_2x2": ([[0, 1, 2, 0], [1, 0, 1, 0], [2, 1, 0, 2], [0, 0, 2, 0]], lambda A, r: r["npiv"][0] == 2),
    # the largest off-diagonal magnitude at (3, 0), (4, 0) and (2, 1): column 0 wins although (2, 1) has the lower row, then row 3
    "offdiag_tie_column_then_row": ([[0, 0, 0, 0, 0], [N_, 0, 0, 0, 0], [N_, 2, 0, 0, 0], [2, N_, N_, 0, 0], [2, N_, N_, N_, 0]],
                                    lambda A, r: first_offdiag(A) == ((3, 0), 3) and r["npiv"][0] == 2 and list(r["perm_fwd"][:2]) == [0, 3]
                                    and np.count_nonzero(np.tril(A, -1)) >= 6),
    # the largest diagonal magnitude at 1 and 3: the first one is the pivot
    "diagonal_tie": ([[1, 0, 0, 0], [N_, -4, 0, 0], [N_, N_, 2, 0], [N_, N_, N_, 4]],
                     lambda A, r: r["npiv"][0] == 1 and r["perm_fwd"][0] == 1 and np.count_nonzero(np.tril(A, -1)) >= 3),
    # a 2 x 2 pivot (i0, i1) = (1, 2): the second swap moves the row that the first one has just placed at position 1
    "second_swap_moves_first": ([[0, 0, 0, 0], [N_, 0, 0, 0], [N_, 2, 0, 0], [N_, N_, N_, 0]],
                                lambda A, r: first_offdiag(A)[0] == (2, 1) and r["npiv"][0] == 2 and list(r["perm_fwd"][:2]) == [1, 2]
                                and np.count_nonzero(np.tril(A, -1)) >= 4),
    # a diagonal matrix with unsorted magnitudes (one tie): the tail alone
    "diagonal_unsorted": (D4.tolist(), lambda A, r: r["tail_from"] == 0 and list(r["perm_fwd"]) == [1, 2, 4, 0, 3]),
    # blockdiag(B, D): the main loop ends early, the tail finishes
    "blockdiag_early_exit": (np.block([[P3, np.zeros((3, 4))], [np.zeros((4, 3)), np.diag([1.0, 0.0, -2.0, 0.5])]]).tolist(),
                             lambda A, r: 0 < r["tail_from"] < 5),
    "zero": (np.zeros((3, 3)).tolist(),
             lambda A, r: r["tail_from"] == 0 and r["transposition_count"] == 0 and not r["packed"].any() and not r["subdiag"].any()),
}

cases = {}
for name, (template, accept) in TEMPLATES.items():
    A, r = fill(template, accept)
    assert np.array_equal(A, A.T)
    cases[name] = {"a": A.tolist(),
                   "expected": {"packed": r["packed"].tolist(), "subdiag": r["subdiag"].tolist(), "perm_fwd": [int(v) for v in r["perm_fwd"]],
                                "transposition_count": int(r["transposition_count"]), "npiv": r["npiv"], "tail_from": int(r["tail_from"])}}

seeds = {}
for n in PARITY_SIZES:
    for seed in range(100):
        if fref.lblt_full(ref.random_symmetric(n, seed))["margin"] >= MARGIN:
            seeds[str(n)] = {"seed": seed, "candidates_rejected": seed}
            break
    else:
        raise SystemExit(f"no seed with margin >= {MARGIN} at n = {n}")
out = {"source": "exact cases of the Full pivoting strategy and parity seeds; expected values from tests/lblt_full_ref.py, verified exactly",
       "margin": MARGIN, "cases": cases, "parity_seeds": seeds}
with open(os.path.join(HERE, "lblt_full_cases.json"), "w") as f:
    json.dump(out, f, indent=1)
print(seeds)
for k, v in cases.items():
    print(k, v["a"], v["expected"]["npiv"], v["expected"]["perm_fwd"], v["expected"]["tail_from"])
