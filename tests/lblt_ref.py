"""NumPy restatement (float64) of the Bunch-Kaufman factorization P A P^T = L B L^T that include/faer_hip.h section 2g specifies:
the unblocked algorithm with the four pivoting strategies, the solve and the reconstruction.  Written from the description of
the algorithm, for the tests only.

Pivot rule, alpha = (1 + sqrt(17)) / 8.  gamma(i) = largest |a| over the off-diagonal of symmetric column i of the current trailing
matrix, ties to the lowest index.  i0 = first arg-max of the trailing diagonal (PartialDiag / RookDiag) or the first trailing index.
  * gamma(i0) == 0 or one row left: 1 x 1 step without elimination.
  * |a[i0, i0]| >= alpha gamma(i0): 1 x 1 pivot i0.
  * otherwise i1 = arg-max of column i0.  Partial: |a[i0, i0]| >= alpha gamma(i1)^2 / gamma(i0): 1 x 1 pivot i0; |a[i1, i1]| >= alpha
    gamma(i1): 1 x 1 pivot i1; else the 2 x 2 pivot (i0, i1).  Rook: |a[i1, i1]| >= alpha gamma(i1): 1 x 1 pivot i1; the arg-max of
    column i1 is i0 again, or gamma(i1) == gamma(i0): 2 x 2 pivot (i0, i1); else move on to (i1, arg-max of column i1).

Besides the factors every run returns its minimum relative decision margin: the smallest relative gap between the two sides of any
comparison that decided a pivot (arg-max winner against runner-up, |a_ii| against alpha gamma, ...).  A run whose margin is far
above the rounding differences between two implementations must give the same pivots in both."""
import math

import numpy as np

ALPHA = (1.0 + math.sqrt(17.0)) / 8.0
STRATEGIES = {"partial": (0, False, False), "partial_diag": (1, False, True), "rook": (2, True, False), "rook_diag": (3, True, True)}


class _Margin:
    def __init__(self):
        self.value = math.inf

    def cmp(self, a, b):
        """records the relative gap of the comparison of a with b"""
        s = max(abs(a), abs(b))
        if s > 0:
            self.value = min(self.value, abs(a - b) / s)

    def argmax(self, vals):
        """first arg-max of vals; records the gap between the winner and the runner-up"""
        i = int(np.argmax(vals))  # numpy returns the first of equal maxima
        if len(vals) > 1:
            rest = np.delete(vals, i)
            self.cmp(vals[i], rest.max())
        return i, float(vals[i])


def _sym_swap(a, l, p, q):
    if p == q:
        return
    a[[p, q], :] = a[[q, p], :]
    a[:, [p, q]] = a[:, [q, p]]
    l[[p, q], :] = l[[q, p], :]


def lblt_unblocked(A, strategy="partial_diag"):
    """A: symmetric, only its lower triangle is read.  Returns a dict: L (unit lower), d (diagonal of B), subdiag, perm_fwd, perm_bwd,
    transposition_count, npiv (1 / 2 per step), margin, packed (what the in-place routine leaves in the lower triangle)."""
    _, rook, diagonal = STRATEGIES[strategy]
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    a = np.tril(A) + np.tril(A, -1).T
    l = np.zeros((n, n))
    sub = np.zeros(n)
    piv = np.arange(n)
    npivs = []
    mg = _Margin()

    def offdiag(k, idx):
        rows = np.array([r for r in range(k, n) if r != idx], dtype=int)
        if len(rows) == 0:
            return None, 0.0
        j, g = mg.argmax(np.abs(a[rows, idx]))
        return int(rows[j]), g

    k = 0
    while k < n:
        i0 = k
        if diagonal:
            i0 = k + mg.argmax(np.abs(np.diag(a)[k:]))[0]
        i1 = None
        npiv = 1
        nothing = False
        r, gamma_i = offdiag(k, i0)
        if k + 1 == n or gamma_i == 0.0:
            nothing = True
        else:
            mg.cmp(abs(a[i0, i0]), ALPHA * gamma_i)
            if abs(a[i0, i0]) >= ALPHA * gamma_i:
                pass
            else:
                i1 = r
                if rook:
                    while True:
                        s, gamma_r = offdiag(k, i1)
                        mg.cmp(abs(a[i1, i1]), ALPHA * gamma_r)
                        if abs(a[i1, i1]) >= ALPHA * gamma_r:
                            i0, i1 = i1, None
                            break
                        if s == i0:
                            npiv = 2
                            break
                        mg.cmp(gamma_i, gamma_r)
                        if gamma_i == gamma_r:
                            npiv = 2
                            break
                        i0, i1, gamma_i = i1, s, gamma_r
                else:
                    _, gamma_r = offdiag(k, i1)
                    rhs = (ALPHA * gamma_r) * (gamma_r / gamma_i)
                    mg.cmp(abs(a[i0, i0]), rhs)
                    if abs(a[i0, i0]) >= rhs:
                        i1 = None
                    else:
                        mg.cmp(abs(a[i1, i1]), ALPHA * gamma_r)
                        if abs(a[i1, i1]) >= ALPHA * gamma_r:
                            i0, i1 = i1, None
                        else:
                            npiv = 2
        if npiv == 2 and i0 > i1:
            i0, i1 = i1, i0
        _sym_swap(a, l, k, i0)
        piv[k] = i0
        if npiv == 2:
            _sym_swap(a, l, k + 1, i1)
            piv[k + 1] = i1
        if nothing:
            pass
        elif npiv == 1:
            d = a[k, k]
            dinv = 1.0 / d
            x = a[k + 1:, k].copy()
            w = x * dinv
            t = np.tril(a[k + 1:, k + 1:] - np.outer(x, w))
            a[k + 1:, k + 1:] = t + np.tril(t, -1).T
            l[k + 1:, k] = w
        else:
            a00, a11, a10 = a[k, k], a[k + 1, k + 1], a[k + 1, k]
            sub[k] = a10
            d10_inv = 1.0 / abs(a10)
            d00, d11 = a00 * d10_inv, a11 * d10_inv
            t = 1.0 / (d00 * d11 - 1.0)
            d10 = a10 * d10_inv
            d = t * d10_inv
            x0, x1 = a[k + 2:, k].copy(), a[k + 2:, k + 1].copy()
            w0 = (x0 * d11 - x1 * d10) * d
            w1 = (x1 * d00 - x0 * d10) * d
            t = np.tril(a[k + 2:, k + 2:] - np.outer(x0, w0) - np.outer(x1, w1))
            a[k + 2:, k + 2:] = t + np.tril(t, -1).T
            l[k + 2:, k] = w0
            l[k + 2:, k + 1] = w1
        npivs.append(npiv)
        k += npiv
    perm = np.arange(n)
    count = 0
    for i in range(n):
        if piv[i] != i:
            count += 1
        perm[[i, piv[i]]] = perm[[piv[i], i]]
    bwd = np.empty(n, dtype=int)
    bwd[perm] = np.arange(n)
    dvec = np.diag(a).copy()
    L = l + np.eye(n)
    return {"L": L, "d": dvec, "subdiag": sub, "perm_fwd": perm, "perm_bwd": bwd, "transposition_count": count, "npiv": npivs,
            "margin": mg.value, "packed": np.tril(l, -1) + np.diag(dvec)}


def block_diag(d, sub):
    n = len(d)
    B = np.diag(np.asarray(d, dtype=np.float64))
    for j in range(n - 1):
        if sub[j] != 0:
            B[j + 1, j] = B[j, j + 1] = sub[j]
    return B


def unit_lower(packed):
    p = np.asarray(packed, dtype=np.float64)
    return np.tril(p, -1) + np.eye(p.shape[0])


def lblt_reconstruct(L, d, sub, perm_fwd):
    """A with (P A P^T)[i, j] = A[perm_fwd[i], perm_fwd[j]] = (L B L^T)[i, j]"""
    M = L @ block_diag(d, sub) @ L.T
    n = len(d)
    bwd = np.empty(n, dtype=int)
    bwd[np.asarray(perm_fwd, dtype=int)] = np.arange(n)
    return M[np.ix_(bwd, bwd)]


def lblt_solve(L, d, sub, perm_fwd, rhs):
    """permute, unit lower solve, block diagonal solve (1 x 1: reciprocal; 2 x 2: the scaled form), unit upper solve, permute back"""
    n = len(d)
    pf = np.asarray(perm_fwd, dtype=int)
    x = np.array(rhs, dtype=np.float64).reshape(n, -1)[pf]
    for j in range(n):
        x[j + 1:] -= np.outer(L[j + 1:, j], x[j])
    i = 0
    while i < n:
        if i + 1 >= n or sub[i] == 0:
            x[i] *= 1.0 / d[i]
            i += 1
        else:
            akp1k = 1.0 / sub[i]
            ak, akp1 = akp1k * d[i], akp1k * d[i + 1]
            denom = 1.0 / (ak * akp1 - 1.0)
            xk, xkp1 = x[i] * akp1k, x[i + 1] * akp1k
            x[i], x[i + 1] = (akp1 * xk - xkp1) * denom, (ak * xkp1 - xk) * denom
            i += 2
    for j in range(n - 1, -1, -1):
        x[:j] -= np.outer(L[j, :j], x[j])
    out = np.empty_like(x)
    out[pf] = x
    return out.reshape(np.shape(rhs))


def random_symmetric(n, seed):
    """the seeded Gaussian symmetric test matrix"""
    g = np.random.default_rng(seed).standard_normal((n, n))
    return (g + g.T) / 2.0


def kkt(n, seed):
    """[[H, B^T], [B, 0]] with H SPD (n - n // 3 rows) and B Gaussian: many 2 x 2 pivots"""
    rng = np.random.default_rng(seed)
    q = n // 3
    p = n - q
    g = rng.standard_normal((p, p))
    H = g @ g.T / p + 0.1 * np.eye(p)
    B = rng.standard_normal((q, p))
    K = np.zeros((n, n))
    K[:p, :p] = H
    K[p:, :p] = B
    K[:p, p:] = B.T
    return K
