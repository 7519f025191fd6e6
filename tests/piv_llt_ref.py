"""NumPy float64 restatement of the Cholesky factorization with diagonal pivoting (include/faer_hip.h section 2h), written from its
specification: P A P^T = L L^T, every step takes the first strict maximum of the updated diagonal a_ii - sum_c l_ic^2 as its pivot,
a negative / NaN diagonal entry of A gives NonPositivePivot{0}, a NaN in the updated diagonal at step j NonPositivePivot{j}, and from
step 1 on a pivot below tol = eps * n * max diag(A) ends the factorization with rank = j.  Unblocked; only the lower triangle of A is
read.  Besides the factors it reports how close every decision of the run was, so that a test can tell a rounding-sensitive input
from a wrong implementation."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps


def spd(n, seed):
    """G G^T + n I, the full-rank input of the tests"""
    g = np.random.default_rng(seed).standard_normal((n, n))
    return g @ g.T + n * np.eye(n)


def low_rank(n, seed):
    """G G^T with G n x floor(n / 2): positive semidefinite of rank floor(n / 2)"""
    g = np.random.default_rng(seed).standard_normal((n, n // 2))
    return g @ g.T


def _first_strict_max(d, start):
    """(index, value, runner-up value) of the first strict maximum above 0 of d[start:]; index `start`, value 0 when nothing is
    positive.  The runner-up is the largest candidate at another index (-inf: none)."""
    pvt, best = start, 0.0
    for i in range(start, len(d)):
        if d[i] > best:
            pvt, best = i, d[i]
    others = [d[i] for i in range(start, len(d)) if i != pvt]
    return pvt, best, (max(others) if others else -math.inf)


def piv_llt_unblocked(a):
    """returns a dict: status ("ok" or "non_positive_pivot"), index (of the error), rank, transposition_count, perm_fwd, perm_bwd,
    L (n x n, columns >= rank zero), packed (the lower triangle as the factorization leaves it: columns < rank of L and the exit
    pivot at [rank, rank]; everything else is the permuted input and unspecified), margin (the minimum over the accepted steps of
    (winner - runner-up) / winner of the arg-max; inf when no step had a choice) and exit_ratio (exit pivot / tol at an early stop,
    else None)"""
    w = np.array(a, dtype=np.float64)
    n = w.shape[0]
    w = np.tril(w) + np.tril(w, -1).T  # the lower triangle is the matrix
    perm = np.arange(n)
    out = {"status": "ok", "index": None, "rank": n, "transposition_count": 0, "margin": math.inf, "exit_ratio": None}

    def finish():
        out["perm_fwd"] = perm.copy()
        out["perm_bwd"] = np.argsort(perm)
        L = np.tril(w)
        L[:, out["rank"]:] = 0
        out["L"] = L
        out["packed"] = np.tril(w)
        return out

    if n == 0:
        return finish()
    d0 = np.diag(w).copy()
    if np.any(np.isnan(d0)) or np.any(d0 < 0):
        out.update(status="non_positive_pivot", index=0, rank=0)
        return finish()
    tol = EPS * n * max(d0.max(), 0.0)
    s = np.zeros(n)  # running sums of squares of the rows of L
    for j in range(n):
        d = np.diag(w) - s
        if np.any(np.isnan(d[j:])):
            out.update(status="non_positive_pivot", index=j, rank=0)
            return finish()
        pvt, ajj, second = _first_strict_max(d, j)
        if j > 0 and ajj < tol:
            out["rank"] = j
            out["exit_ratio"] = ajj / tol if tol > 0 else 0.0
            w[j, j] = ajj
            return finish()
        if second > -math.inf and ajj > 0:
            out["margin"] = min(out["margin"], (ajj - second) / ajj)
        if pvt != j:
            out["transposition_count"] += 1
            p = np.arange(n)
            p[j], p[pvt] = pvt, j
            w = w[np.ix_(p, p)]
            s[[j, pvt]] = s[[pvt, j]]
            perm[[j, pvt]] = perm[[pvt, j]]
        with np.errstate(divide="ignore", invalid="ignore"):
            root = math.sqrt(ajj)
            col = (w[j + 1:, j] - w[j + 1:, :j] @ w[j, :j]) * (1.0 / root if root != 0 else math.inf)
        w[j, j] = root
        w[j + 1:, j] = col  # (the lower triangle of w: L in the first j + 1 columns, the permuted input right of them)
        s[j + 1:] += col * col
    return finish()


def piv_llt_solve(L, perm_fwd, b):
    """x with A x = b from a full-rank factorization: gather by perm_fwd, two triangular solves, gather by perm_bwd"""
    y = np.linalg.solve(L, np.asarray(b, dtype=np.float64)[perm_fwd])
    z = np.linalg.solve(L.T, y)
    return z[np.argsort(perm_fwd)]


def piv_llt_reconstruct(L, perm_fwd):
    """A = P^T L L^T P"""
    pb = np.argsort(perm_fwd)
    return (L @ L.T)[np.ix_(pb, pb)]
