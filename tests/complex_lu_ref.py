"""Plain numpy yardsticks of the complex partial-pivot LU; no GPU, no library.

lu_unblocked restates the reference's lu_in_place_unblocked (lu/partial_pivoting/factor.rs:19-67) in the working precision: the
pivot of column j is the first row i >= j whose abs1 = |re| + |im| is strictly larger than every earlier candidate's, starting from
0 (an all-zero column keeps row j, a NaN is never chosen); the reciprocal is conj(p) / |p|^2, unscaled; every product and sum
rounds on its own.

The error yardsticks work in clongdouble.  C = 12 is C_TRI_COMPLEX of tests/complex_cases.py: the real constant 4 times the 2 sqrt 2
of complex arithmetic.  Higham, Accuracy and Stability of Numerical Algorithms, Theorem 9.3 bounds |L U - P A| by gamma_k |L||U|
for any order of the inner sums, so the bound holds for the GEMM-updated factorization as for the unblocked one."""
import numpy as np

C = 12


def abs1(z):
    return np.abs(z.real) + np.abs(z.imag)


def _mul(a, b):
    """complex product with every real product and sum rounded on its own, in the real precision of a / b"""
    return (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)


def lu_unblocked(a):
    """(packed LU, perm, transposition count): a[perm] == L U, L unit lower (m x k), U upper (k x n), k = min(m, n)"""
    lu = np.array(a, order="F", copy=True)
    t = lu.dtype.type
    m, n = lu.shape
    perm = np.arange(m)
    count = 0
    with np.errstate(all="ignore"):
        for j in range(min(m, n)):
            # first strict maximum above 0 among the non-NaN candidates (argmax returns the first of equal values)
            col = abs1(lu[j:, j])
            col = np.where(np.isnan(col), -1, col)
            i = int(np.argmax(col))
            p = j + i if col[i] > 0 else j
            if p != j:
                lu[[j, p], :] = lu[[p, j], :]
                perm[[j, p]] = perm[[p, j]]
                count += 1
            piv = lu[j, j]
            den = piv.real * piv.real + piv.imag * piv.imag
            inv = t(piv.real / den + 1j * (-piv.imag / den))
            lu[j + 1:, j] = _mul(lu[j + 1:, j], inv).astype(t)
            lu[j + 1:, j + 1:] -= _mul(lu[j + 1:, j:j + 1], lu[j:j + 1, j + 1:]).astype(t)
    return lu, perm, count


def split(lu):
    m, n = lu.shape
    k = min(m, n)
    l = np.tril(lu[:, :k], -1) + np.eye(m, k, dtype=lu.dtype)
    u = np.triu(lu[:k, :])
    return l, u


def lu_backward_error(a, lu, perm, c=C):
    """max over the entries of |L U - A[perm]| / (c max(k, 1) eps |L||U|); <= 1 passes, non-finite factors give inf"""
    if not np.isfinite(lu).all():
        return np.inf
    eps = np.finfo(lu.dtype).eps
    m, n = lu.shape
    k = min(m, n)
    if m == 0 or n == 0:
        return 0.0
    l, u = split(lu.astype(np.clongdouble))
    res = np.abs(l @ u - a.astype(np.clongdouble)[np.asarray(perm, dtype=np.int64)])
    den = c * max(k, 1) * np.longdouble(eps) * (np.abs(l) @ np.abs(u))
    with np.errstate(all="ignore"):
        q = np.where(res == 0, 0, res / den)
    return float(np.max(q))


def solve_error(opa, absa, x, b, dtype, c=C):
    """max over the entries of |op(A) X - B| / (c 3 n eps (absa |X| + |B|)), absa = |L||U| arranged like op(A); <= 1 passes"""
    if not np.isfinite(x).all():
        return np.inf
    n = opa.shape[0]
    eps = np.longdouble(np.finfo(dtype).eps)
    xl, bl = x.astype(np.clongdouble), b.astype(np.clongdouble)
    res = np.abs(opa.astype(np.clongdouble) @ xl - bl)
    den = c * 3 * max(n, 1) * eps * (absa.astype(np.longdouble) @ np.abs(xl) + np.abs(bl))
    with np.errstate(all="ignore"):
        q = np.where(res == 0, 0, res / den)
    return float(np.max(q))


def abs_lu(lu, perm):
    """|L||U| in the row order of A (so that it stands next to A itself): (P^T |L||U|)"""
    l, u = split(lu.astype(np.clongdouble))
    g = (np.abs(l) @ np.abs(u)).astype(np.longdouble)
    out = np.empty_like(g)
    out[np.asarray(perm, dtype=np.int64)] = g
    return out


def records_from_perm(perm, k):
    """the transposition records (row exchanged with row j, j < k) that build `perm`, and how many are non-trivial"""
    perm = np.asarray(perm, dtype=np.int64)
    cur = np.arange(perm.shape[0])
    where = np.arange(perm.shape[0])  # where[r] = current position of original row r
    rec = []
    for j in range(k):
        p = where[perm[j]]
        rec.append(int(p))
        rj, rp = cur[j], cur[p]
        cur[j], cur[p] = rp, rj
        where[rp], where[rj] = j, p
    assert np.array_equal(cur[:k], perm[:k])
    return rec, sum(1 for j, p in enumerate(rec) if p != j)


# ---- inputs shared by the CPU and GPU tests
def gaussian(m, n, dtype, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))).astype(dtype))


def exact_case(n, dtype, seed=5):
    """(A, L, U) with A = L U exact in complex64 already: L unit lower with entries in {0, +-1, +-i} / 2 below the diagonal, U with
    Gaussian-integer entries in [-1, 1]^2 above a diagonal from {+-4, +-4i}.  Column j of the partly eliminated matrix holds the
    diagonal (abs1 4) and below it l_ij u_jj (abs1 <= 2): the diagonal dominates in abs1, no interchange happens.  Every partial
    sum of A = L U and of the elimination is a multiple of 1 / 2 below 2 n, exact in either precision."""
    rng = np.random.default_rng(seed)
    units = np.array([0, 1, -1, 1j, -1j])
    l = np.tril(units[rng.integers(0, 5, (n, n))] / 2, -1) + np.eye(n)
    u = np.triu(rng.integers(-1, 2, (n, n)) + 1j * rng.integers(-1, 2, (n, n)), 1)
    u = u + np.diag(4 * units[rng.integers(1, 5, n)])
    a = l @ u
    return np.asfortranarray(a.astype(dtype)), np.asfortranarray(l.astype(dtype)), np.asfortranarray(u.astype(dtype))
