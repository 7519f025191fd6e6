"""The reference's three routines that modify a Cholesky factorization, restated in numpy in the working precision of their
operands (real scalars): cholesky/llt/update.rs:271-345 and :360 (rank_r_update_clobber), cholesky/ldlt/update.rs:244-320 and :376,
delete_rows_and_cols_clobber (:417) with rank_update_indices (:322) and delete_rows_and_cols_triangular (:343).  Every scalar
operation is done in the dtype of `l`; the two row updates are fused multiply-adds like the reference's (emulated in longdouble,
which is exact for fp32 and within a fraction of an ulp for fp64 -- the tests compare against tolerances, not bits).

Also the input families shared by the host and GPU tests (case_update, case_delete)."""
import numpy as np


class NonPositivePivot(Exception):
    def __init__(self, index):
        super().__init__(f"NonPositivePivot {{ index: {index} }}")
        self.index = index


def _fma(a, b, c, dt):
    return (np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble) + np.asarray(c, np.longdouble)).astype(dt)


def _run(l, w, alpha, ldlt, r_of):
    """RankRUpdate::run: column j sees the first r_of() columns of w"""
    dt = l.dtype.type
    n, kk = w.shape
    assert l.shape == (n, n) and alpha.shape == (kk,) and w.dtype == l.dtype and alpha.dtype == l.dtype
    with np.errstate(all="ignore"):
        for j in range(n):
            r = min(r_of(), kk)
            for k in range(r):
                d, p = l[j, j], w[j, k]
                ap = dt(alpha[k] * p)
                if ldlt:
                    nd = dt(d + dt(ap * p))
                    if d == 0 and nd == 0:
                        beta, pneg = dt(0), -dt(0)
                    else:
                        beta = dt(ap * dt(dt(1) / nd))
                        alpha[k] = dt(alpha[k] - dt(nd * dt(beta * beta)))
                        pneg = dt(-p)
                    gamma = None
                else:
                    nd2 = dt(dt(d * d) + dt(ap * p))
                    if nd2 <= 0:
                        raise NonPositivePivot(j)
                    nd = dt(np.sqrt(nd2))
                    dinv, ndinv = dt(dt(1) / d), dt(dt(1) / nd)
                    gamma, beta, pneg = dt(nd * dinv), dt(ap * ndinv), dt(-dt(p * dinv))
                    alpha[k] = dt(alpha[k] - dt(beta * beta))
                l[j, j] = nd
                if j + 1 < n:
                    w[j + 1:, k] = _fma(pneg, l[j + 1:, j], w[j + 1:, k], dt)
                    l[j + 1:, j] = _fma(beta, w[j + 1:, k], l[j + 1:, j] if ldlt else (gamma * l[j + 1:, j]).astype(dt), dt)


def llt_rank_r_update_clobber(l, w, alpha):
    """in place on the lower triangle of `l`; raises NonPositivePivot(index)"""
    r = w.shape[1]
    _run(l, w, alpha, False, lambda: r)


def ldlt_rank_r_update_clobber(ld, w, alpha):
    r = w.shape[1]
    _run(ld, w, alpha, True, lambda: r)


def rank_update_indices(start_col, indices):
    """update.rs:322-342: a callable that returns, call after call, how many columns of w the next column of the block sees"""
    state = {"col": start_col, "r": 0}

    def nxt():
        if state["r"] == len(indices):
            return state["r"]
        while state["col"] == indices[state["r"]] - state["r"]:
            state["r"] += 1
            if state["r"] == len(indices):
                return state["r"]
        state["col"] += 1
        return state["r"]

    return nxt


def delete_rows_and_cols_triangular(a, idx):
    """update.rs:343-374"""
    n, r = a.shape[0], len(idx)
    for cj in range(r + 1):
        j0 = 0 if cj == 0 else idx[cj - 1] + 1
        j1 = n if cj == r else idx[cj]
        for j in range(j0, j1):
            for ci in range(cj, r + 1):
                i0 = j if ci == cj else idx[ci - 1] + 1
                i1 = n if ci == r else idx[ci]
                if (ci != 0 or cj != 0) and i1 > i0:
                    a[i0 - ci:i1 - ci, j - cj] = a[i0:i1, j]


def ldlt_delete_rows_and_cols_clobber(ld, indices):
    """update.rs:417-461; returns the sorted indices.  The leading (n - r)^2 block of `ld` receives the factors."""
    n, r = ld.shape[0], len(indices)
    if r == 0:
        return []
    idx = sorted(int(i) for i in indices)
    assert all(idx[i + 1] > idx[i] for i in range(r - 1)) and idx[-1] < n
    first = idx[0]
    m = n - first - r
    w = np.full((m, r), np.nan, dtype=ld.dtype)  # (uninit in the reference: what is never written is never read)
    alpha = np.empty(r, dtype=ld.dtype)
    for k in range(r):
        j = idx[k]
        alpha[k] = ld[j, j]
        for ci in range(k + 1, r + 1):
            i0 = idx[ci - 1] + 1
            i1 = n if ci == r else idx[ci]
            if i1 > i0:
                w[i0 - ci - first:i1 - ci - first, k] = ld[i0:i1, j]
    delete_rows_and_cols_triangular(ld, idx)
    _run(ld[first:first + m, first:first + m], w, alpha, True, rank_update_indices(first, idx))
    return idx


# ---- what the factors stand for
def llt_product(l):
    t = np.tril(l).astype(np.float64)
    return t @ t.T


def ldlt_product(ld):
    t = np.tril(ld, -1).astype(np.float64) + np.eye(ld.shape[0])
    return (t * np.diag(ld).astype(np.float64)) @ t.T


def llt_factor(a):
    return np.linalg.cholesky(a.astype(np.float64))


def ldlt_factor(a):
    """unit lower L strictly below the diagonal, D on it (of a positive definite matrix, from its Cholesky factor)"""
    c = np.linalg.cholesky(a.astype(np.float64))
    d = np.diag(c)
    ld = np.tril(c / d, -1)
    ld[np.diag_indices_from(ld)] = d * d
    return ld


def residual_bound(n, a, dtype):
    """64 n eps max|A|; `a`: the matrix, or max|A| itself"""
    return 64 * n * np.finfo(dtype).eps * np.abs(a).max()


# ---- the input families of the tests
def case_update(n, r, dtype, ldlt, downdate, seed=0):
    """(factor, w, alpha, target, amax): A = G G^T + n I, W standard normal, |alpha| in [0.1, inf); the factor handed over is that of A
    for an update (alpha > 0) and that of A_big = A + W |alpha| W^T for a downdate (alpha < 0); `target` (fp64) is what the new factor
    stands for.  `amax` is the max|A| of the residual bound: the largest entry of the larger of the two matrices, A_big in both
    directions.  A downdate's data is the factor of A_big, whose rounding alone moves the result by eps max|A_big|; measured against
    max|A| of the small matrix the restatement itself reaches 84 n eps at n = 1, r = 31 (fp64) and 414 n eps in fp32, against
    max|A_big| it stays below 4.2 n eps on every size of the tests in both precisions."""
    rng = np.random.default_rng(1000 * n + 10 * r + 2 * int(ldlt) + int(downdate) + seed)
    g = rng.standard_normal((n, n))
    a = g @ g.T + n * np.eye(n)
    w = rng.standard_normal((n, r)).astype(dtype)
    mag = (0.1 + rng.exponential(1.0, r)).astype(dtype)
    wa = (w.astype(np.float64) * mag.astype(np.float64)) @ w.astype(np.float64).T
    start, target, alpha = (a + wa, a, -mag) if downdate else (a, a + wa, mag)
    f = (ldlt_factor if ldlt else llt_factor)(start).astype(dtype)
    # what the rounded factor stands for, so that the residual measures the update alone
    start_r = (ldlt_product if ldlt else llt_product)(f)
    target = start_r - wa if downdate else start_r + wa
    return np.asfortranarray(f), np.asfortranarray(w), alpha.copy(), target, max(np.abs(start_r).max(), np.abs(target).max())


def index_sets(n):
    """the deletion index sets of the tests: (name, indices as handed over)"""
    sets = [("first", [0]), ("last", [n - 1]), ("ends", sorted({0, 1, n // 2, n - 1})), ("seventh", list(range(0, n, 7))[:9])]
    if n // 2 > 1:
        sets.append(("two", [1, n // 2]))
    if n >= 8:
        sets.append(("unsorted", [n // 2, 1, n - 2, 3]))
    else:
        sets.append(("unsorted", [n - 1, 0]))
    return sets


def case_delete(n, dtype, seed=0):
    """(ld, a): the L D L^T factors (in `dtype`) of a positive definite matrix and what they stand for (fp64)"""
    rng = np.random.default_rng(77 * n + seed)
    g = rng.standard_normal((n, n))
    ld = np.asfortranarray(ldlt_factor(g @ g.T + n * np.eye(n)).astype(dtype))
    return ld, ldlt_product(ld)
