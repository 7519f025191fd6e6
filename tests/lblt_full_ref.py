"""NumPy restatement (float64) of the Full pivoting strategy of the Bunch-Kaufman factorization P A P^T = L B L^T that
include/faer_hip.h section 2g specifies; a sibling of tests/lblt_ref.py (the other four strategies), written from the description
of the algorithm, for the tests only.  Only the lower triangle of the input is read.  "abs2" is the square of the magnitude; every
comparison is made on squares.

 1. scale = largest |a_ij| of the lower triangle, diagonal included; the lower triangle is multiplied by 1 / scale (one reciprocal,
    then products).  scale == 0: nothing is scaled.
 2. (max_i, max_j, max_offdiag) = first arg-max of abs2 over the strict lower triangle in column-major order (strict >: ties go to
    the lowest column, then the lowest row).
 3. while k < n and max_offdiag != 0: max_s = first arg-max of abs2 of the trailing diagonal.  alpha = ((1 + sqrt 17) / 8)^2.
    max_diag >= alpha max_offdiag: the 1 x 1 pivot max_s, else the 2 x 2 pivot (i0, i1) = (max_j, max_i).  Symmetric swap of trailing
    position 0 with i0, then (2 x 2) of position 1 with i1, the same rows in the columns on the left.  1 x 1: L = column (1 / d),
    a_ii -= d l_i^2, a_ij -= (l_i l_j) d.  2 x 2: the scaled d00, d11, d10, t form, w0 / w1 per row, a_ij -= x0_i w0_j + x1_i w1_j,
    L0 = w0, L1 = w1.  The arg-max of the next step is that of the updated strict lower triangle; one row left: max_offdiag = 0.
 4. once max_offdiag == 0: every remaining step exchanges the first largest (abs2) trailing diagonal entry with the leading one,
    and the two rows of the columns on the left; nothing is eliminated.
 5. the diagonal and subdiag are multiplied by scale.

Besides the factors every run returns its minimum relative decision margin: the smallest relative gap between every arg-max winner
and its runner-up and between max_diag and alpha max_offdiag.  max_offdiag is compared with 0 through exact zeros only (a nonzero
entry whose square underflows would count as a margin of 0)."""
import math

import numpy as np

ALPHA2 = ((1.0 + math.sqrt(17.0)) * 0.125) ** 2


class _Margin:
    def __init__(self):
        self.value = math.inf

    def cmp(self, a, b):
        s = max(abs(a), abs(b))
        if s > 0:
            self.value = min(self.value, abs(a - b) / s)

    def first_argmax(self, vals):
        """first arg-max of a 1-D array (0, value 0 for an array without a positive entry); records winner against runner-up"""
        if len(vals) == 0:
            return 0, 0.0
        i = int(np.argmax(vals))  # numpy returns the first of equal maxima
        if not vals[i] > 0:
            return 0, 0.0
        if len(vals) > 1:
            self.cmp(vals[i], np.delete(vals, i).max())
        return i, float(vals[i])


def _offdiag_argmax(a, k, mg):
    """first largest abs2 of the strict lower triangle of a[k:, k:] in column-major order: (i, j, value), relative to k"""
    m = a.shape[0] - k
    if m < 2:
        return 0, 0, 0.0
    jj, ii = np.triu_indices(m, 1)  # (column, row) pairs in column-major order of the lower triangle: j ascending, then i ascending
    t = a[k:, k:]
    vals = t[ii, jj] ** 2
    if np.any((t[ii, jj] != 0) & (vals == 0)):
        mg.value = 0.0  # a nonzero entry whose square underflows: "max_offdiag == 0" would not be decided by exact zeros
    p, v = mg.first_argmax(vals)
    if v == 0.0:
        return 0, 0, 0.0
    return int(ii[p]), int(jj[p]), v


def _sym_swap(a, l, p, q):
    if p == q:
        return
    a[[p, q], :] = a[[q, p], :]
    a[:, [p, q]] = a[:, [q, p]]
    l[[p, q], :] = l[[q, p], :]


def lblt_full(A):
    """A: symmetric, only its lower triangle is read.  Returns a dict: L (unit lower), d (diagonal of B), subdiag, perm_fwd, perm_bwd,
    transposition_count, npiv (1 / 2 per step, tail steps count as 1), tail_from (first k of the tail, n if none), margin, packed
    (what the in-place routine leaves in the lower triangle)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    a = np.tril(A) + np.tril(A, -1).T
    l = np.zeros((n, n))
    sub = np.zeros(n)
    piv = np.arange(n)
    npivs = []
    mg = _Margin()
    scale = float(np.abs(a).max()) if n else 0.0
    if scale != 0.0:
        a = a * (1.0 / scale)
    max_i, max_j, max_off = _offdiag_argmax(a, 0, mg)
    k = 0
    while k < n and max_off != 0.0:
        s, max_diag = mg.first_argmax(np.diag(a)[k:] ** 2)
        mg.cmp(max_diag, ALPHA2 * max_off)
        if max_diag >= ALPHA2 * max_off:
            npiv, i0, i1 = 1, s, None
        else:
            npiv, i0, i1 = 2, max_j, max_i
        _sym_swap(a, l, k, k + i0)
        piv[k] = k + i0
        if npiv == 2:
            _sym_swap(a, l, k + 1, k + i1)
            piv[k + 1] = k + i1
        if npiv == 1:
            d = a[k, k]
            lc = a[k + 1:, k] * (1.0 / d)
            t = a[k + 1:, k + 1:]
            new = t - np.outer(lc, lc) * d
            new[np.diag_indices_from(new)] = np.diag(t) - d * lc ** 2
            a[k + 1:, k + 1:] = np.tril(new) + np.tril(new, -1).T
            l[k + 1:, k] = lc
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
            new = a[k + 2:, k + 2:] - np.outer(x0, w0) - np.outer(x1, w1)
            a[k + 2:, k + 2:] = np.tril(new) + np.tril(new, -1).T
            a[k + 1, k] = a[k, k + 1] = 0.0
            l[k + 2:, k] = w0
            l[k + 2:, k + 1] = w1
        npivs.append(npiv)
        k += npiv
        max_i, max_j, max_off = _offdiag_argmax(a, k, mg)
    tail_from = k
    while k < n:
        s, _ = mg.first_argmax(np.diag(a)[k:] ** 2)
        if s != 0:
            a[k, k], a[k + s, k + s] = a[k + s, k + s], a[k, k]
            l[[k, k + s], :] = l[[k + s, k], :]
        piv[k] = k + s
        npivs.append(1)
        k += 1
    perm = np.arange(n)
    count = 0
    for i in range(n):
        if piv[i] != i:
            count += 1
        perm[[i, piv[i]]] = perm[[piv[i], i]]
    bwd = np.empty(n, dtype=int)
    bwd[perm] = np.arange(n)
    dvec = np.diag(a) * scale if scale != 0.0 else np.diag(a).copy()
    sub = sub * scale if scale != 0.0 else sub
    return {"L": l + np.eye(n), "d": dvec, "subdiag": sub, "perm_fwd": perm, "perm_bwd": bwd, "transposition_count": count, "npiv": npivs,
            "tail_from": tail_from, "margin": mg.value, "packed": np.tril(l, -1) + np.diag(dvec)}
