"""Inputs and verdicts of the general EVD tests (tests/test_gpu_evd_general.py on the GPU, tests/test_schur_host.py on the host
build of the same bodies, tests/test_evd_cases.py for this module alone).  Pure numpy, no GPU.

Verdicts.
  column_residuals   |A v_i - l_i v_i|_2 / (|A|_F |v_i|_2) per column.  The back substitution of the EVD does not normalise: the
                     columns of one call differ in norm by up to 1 / sqrt(min positive), and a quotient of Frobenius norms sees
                     only the largest of them.
  assign_spectrum    a one-to-one assignment of the computed eigenvalues to those of a reference, each within the radius of its
                     reference value.  A residual cannot tell a complete spectrum from one with an eigenpair reported twice.

Inputs.  The six kinds of the first EVD tests (normal or random) and the non-normal ones that reach the rest of eigvec_block
(csrc/schur_core.h): the overflow guard at its four places (a real column or a pair's two columns, over a 1 x 1 or a 2 x 2
diagonal block), the divisor floor (repeated eigenvalues in a non-diagonal T), and dense inputs with the same Schur forms."""
import numpy as np

DTYPES = [np.float64, np.float32]
KINDS = ["normal01", "symmetric", "triangular", "block_diagonal", "cyclic", "normal"]
TRIANGULAR_KINDS = ["graded_triangular", "graded_quasi", "jordan", "repeated_blocks"]
DEFECTIVE = {"jordan", "repeated_blocks"}
NEW_KINDS = TRIANGULAR_KINDS + ["rotated_" + k for k in TRIANGULAR_KINDS] + ["scaled_similarity"]

# rows of the unrotated graded kinds per dtype: the guard fires in graded_triangular, and at all four of its places in
# graded_quasi (tests/test_evd_cases.py asserts both in extended precision); one leaf of the device code
GUARD_N = {np.dtype(np.float64): 96, np.dtype(np.float32): 96}


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def guard_threshold(dtype):
    """1 / sqrt(min positive): eigvec_guard rescales a vector when a new component passes it"""
    return 1.0 / float(np.sqrt(np.float64(np.finfo(dtype).tiny)))


def make(kind, n, dtype, seed=0):
    """(matrix, known eigenvalues or None) of the six normal or random kinds"""
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "normal01":
        return np.asarray(rng.standard_normal((n, n)), dtype=dtype), None
    if kind == "symmetric":
        x = rng.standard_normal((n, n))
        return np.asarray(x + x.T, dtype=dtype), None
    if kind == "triangular":
        return np.asarray(np.triu(rng.standard_normal((n, n))), dtype=dtype), None
    if kind == "block_diagonal":
        a = np.zeros((n, n))
        cuts = sorted({0, min(n, max(1, n // 7)), min(n, max(2, n // 7 + (2 * n) // 3)), n})  # unequal blocks, the first one small
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            a[lo:hi, lo:hi] = rng.standard_normal((hi - lo, hi - lo))
        return np.asarray(a, dtype=dtype), None
    if kind == "cyclic":
        a = np.zeros((n, n))
        a[np.arange(1, n), np.arange(n - 1)] = 1.0
        a[0, n - 1] = 1.0
        return np.asarray(a, dtype=dtype), np.exp(2j * np.pi * np.arange(n) / n)
    if kind == "normal":
        b = np.zeros((n, n))
        lam = []
        i = 0
        while i < n:
            if i + 1 < n and rng.random() < 0.6:
                x, y = rng.standard_normal(2)
                b[i:i + 2, i:i + 2] = [[x, y], [-y, x]]
                lam += [x + 1j * y, x - 1j * y]
                i += 2
            else:
                b[i, i] = rng.standard_normal()
                lam.append(b[i, i] + 0j)
                i += 1
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return np.asarray(q @ b @ q.T, dtype=dtype), np.array(lam)
    raise ValueError(kind)


def quasi_spectrum(t):
    """eigenvalues of a quasi upper triangular matrix whose 2 x 2 blocks are standardised, in the order of its diagonal"""
    t = np.asarray(t, dtype=np.float64)
    n = t.shape[0]
    lam = np.diag(t).astype(complex)
    for i in np.nonzero(np.diag(t, -1))[0]:
        q = np.sqrt(abs(t[i, i + 1])) * np.sqrt(abs(t[i + 1, i]))
        lam[i] += 1j * q
        lam[i + 1] -= 1j * q
    assert lam.shape == (n,)
    return lam


def graded_triangular(n, dtype, sup=1e3):
    """diagonal 1 + i 1e-3, first and second superdiagonals 1e3: an eigenvector grows by about 1e6 / j at the j-th row above its own"""
    a = np.diag(1.0 + 1e-3 * np.arange(n))
    for d in (1, 2):
        a += np.diag(np.full(n - d, sup), d) if n > d else 0
    a = np.asarray(a, dtype=dtype)
    return a, np.diag(a).astype(complex), False


def graded_quasi(n, dtype, sup=1e4, y=1.0):
    """graded_triangular with the standard block [[x, y], [-y / 4, x]] (x +- i y / 2) on rows 4 j, 4 j + 1; rows 4 j + 2, 4 j + 3
    stay 1 x 1, so real columns and pairs both meet 1 x 1 and 2 x 2 pivots on the way up.  Superdiagonals 1e4: with 1e3 the fp64
    vectors pass the threshold so rarely that two of the guard's four places stay unreached at any n of one leaf."""
    a = graded_triangular(n, dtype, sup)[0].astype(np.float64)
    for i in range(0, n - 1, 4):
        a[i + 1, i + 1] = a[i, i]
        a[i, i + 1] = y
        a[i + 1, i] = -y / 4
    a = np.asarray(a, dtype=dtype)
    return a, quasi_spectrum(a), False


def jordan(n, dtype):
    """2 I plus a unit superdiagonal: one eigenvector, every divisor of the back substitution is the floor"""
    return np.asarray(2.0 * np.eye(n) + np.diag(np.ones(n - 1), 1), dtype=dtype), np.full(n, 2.0 + 0j), True


def repeated_blocks(n, dtype):
    """the standard block [[1, 2], [-1/2, 1]] (1 +- i) repeated down the diagonal (a last odd row: 1), N(0, 1) above the blocks:
    the floor in the complex solves"""
    rng = np.random.default_rng(7000 + n)
    a = np.triu(rng.standard_normal((n, n)), 1)
    a[np.arange(n), np.arange(n)] = 1.0
    for i in range(0, n - 1, 2):
        a[i, i + 1] = 2.0
        a[i + 1, i] = -0.5
    a = np.asarray(a, dtype=dtype)
    return a, quasi_spectrum(a), True


def rotated(kind, n, dtype):
    """Q T Q^T of a triangular kind with a random orthogonal Q: dense, through Hessenberg reduction, sweeps and leaves.  Rounding
    Q T Q^T moves the eigenvalues of these T far, so the spectrum is unknown and the case counts as defective (residual only)."""
    t = generate(kind, n, dtype)[0].astype(np.float64)
    q, _ = np.linalg.qr(np.random.default_rng(9000 + n).standard_normal((n, n)))
    return np.asarray(q @ t @ q.T, dtype=dtype), None, True


def scaled_similarity(n, dtype):
    """D B D^-1 with B the `normal` kind and D = diag(2^k), k spread over [-10, 10]: an exact similarity of the rounded B, so the
    spectrum is that of B; non-normal, and every condition number is at most cond(D)"""
    b, _ = make("normal", n, dtype)
    k = np.random.default_rng(8000 + n).integers(-10, 11, n)
    if n > 1:
        k[0], k[-1] = -10, 10
    a = np.ldexp(np.ldexp(b.astype(np.float64), k[:, None]), -k[None, :])
    out = np.asarray(a, dtype=dtype)
    assert np.array_equal(out.astype(np.float64), a)  # exact: a power of two moves no mantissa bit (the range is far away)
    return out, np.linalg.eigvals(b.astype(np.float64)), False


def generate(kind, n, dtype, seed=0):
    """(matrix, known spectrum or None, defective flag) of any kind of this module"""
    if kind in KINDS:
        a, known = make(kind, n, dtype, seed)
        return a, known, False
    if kind.startswith("rotated_"):
        return rotated(kind[len("rotated_"):], n, dtype)
    if kind == "scaled_similarity":
        return scaled_similarity(n, dtype)
    if kind in TRIANGULAR_KINDS:
        return globals()[kind](n, dtype)
    raise ValueError(kind)


def unpack(s, si, u):
    """complex eigenvalues and eigenvector columns from the packed layout; asserts the pair layout of S_im"""
    n = s.shape[0]
    lam = s.astype(np.float64) + 1j * si.astype(np.float64)
    V = None if u is None else np.zeros((n, n), complex)
    i = 0
    while i < n:
        if si[i] == 0:
            if u is not None:
                V[:, i] = u[:, i]
            i += 1
        else:
            assert i + 1 < n and si[i] == -si[i + 1] and si[i] > 0 and s[i] == s[i + 1], f"S_im does not hold a pair at {i}"
            if u is not None:
                V[:, i] = u[:, i].astype(np.float64) + 1j * u[:, i + 1].astype(np.float64)
                V[:, i + 1] = V[:, i].conj()
            i += 2
    return lam, V


def frobenius_quotient(a, lam, V, side="right"):
    """|A V - V L|_F / (|A|_F |V|_F): the verdict of the first EVD tests (the left form for side == "left")"""
    a64 = np.asarray(a, dtype=np.float64)
    V = np.asarray(V, dtype=complex)
    lam = np.asarray(lam, dtype=complex)
    r = a64 @ V - V * lam if side == "right" else a64.T @ V - V * lam.conj()
    return float(np.linalg.norm(r) / max(np.linalg.norm(a64) * np.linalg.norm(V), 1e-300))


def column_residuals(a, lam, V, side="right"):
    """per column |A v_i - l_i v_i|_2 / (|A|_F |v_i|_2); side == "left": |v_i^H A - l_i v_i^H|_2 instead.  In fp64, every column
    divided by its own largest entry first, so that neither a product nor a norm overflows and no column weighs on another.  A zero
    or non-finite column has the residual inf."""
    a64 = np.asarray(a, dtype=np.float64)
    V = np.asarray(V, dtype=complex)
    lam = np.asarray(lam, dtype=complex)
    big = np.abs(V).max(axis=0) if V.size else np.zeros(0)
    bad = ~np.isfinite(big) | (big == 0)
    Vs = np.where(bad[None, :], 0.0, V) / np.where(bad, 1.0, big)[None, :]
    # (v^H A - l v^H)^H = A^T v - conj(l) v for a real A
    r = a64 @ Vs - Vs * lam if side == "right" else a64.T @ Vs - Vs * lam.conj()
    den = max(np.linalg.norm(a64), 1e-300) * np.where(bad, 1.0, np.linalg.norm(Vs, axis=0))
    return np.where(bad, np.inf, np.linalg.norm(r, axis=0) / den)


_NUMPY = {}


def numpy_same_dtype(a, key):
    """numpy's eig (LAPACK geev) in the dtype of a, once per key: (eigenvalues, Frobenius quotient, worst column residual)"""
    if key not in _NUMPY:
        w, v = np.linalg.eig(a)
        w, v = w.astype(complex), v.astype(complex)
        _NUMPY[key] = (w, frobenius_quotient(a, w, v), float(column_residuals(a, w, v).max(initial=0.0)))
    return _NUMPY[key]


def bounds(a, key):
    """(Frobenius bound, per-column bound) of a case: 4 max(numpy's own value in the dtype of a, n eps)"""
    n, e = a.shape[0], eps_of(a.dtype)
    _, rf, rc = numpy_same_dtype(a, key)
    return 4 * max(rf, n * e), 4 * max(rc, n * e)


_REFERENCE = {}


def reference_spectrum(a, key):
    """(eigenvalues, radius per eigenvalue) from numpy's eig in fp64 of the dtype-rounded a, once per key.
    radius_i = c n eps(dtype of a) kappa_i |A|_F with kappa_i = |x_i| |y_i| / |y_i^H x_i|, the y_i^H the rows of inv(X);
    c = 4 for fp32 inputs and 8 for fp64 inputs, where the reference's own error is of the same order.  Where X is singular to
    working precision the condition numbers are beyond 1 / eps and the radius is infinite."""
    if key not in _REFERENCE:
        a64 = np.asarray(a, dtype=np.float64)
        n = a64.shape[0]
        w, x = np.linalg.eig(a64)
        with np.errstate(all="ignore"):
            try:
                y = np.linalg.inv(x)  # rows y_i^H, y_i^H x_i = 1
                kappa = np.linalg.norm(x, axis=0) * np.linalg.norm(y, axis=1) / np.abs(np.einsum("ij,ji->i", y, x))
            except np.linalg.LinAlgError:
                kappa = np.full(n, np.inf)
        kappa = np.where(np.isfinite(kappa), np.maximum(kappa, 1.0), np.inf)
        c = 8.0 if a.dtype == np.float64 else 4.0
        _REFERENCE[key] = (w.astype(complex), c * n * eps_of(a.dtype) * kappa * np.linalg.norm(a64))
    return _REFERENCE[key]


def _augmenting_paths(adj):
    """size of a maximum matching of the bipartite graph adj[i, j] (Kuhn's algorithm, iterative)"""
    n = adj.shape[0]
    nbrs = [np.nonzero(adj[i])[0] for i in range(n)]
    owner = -np.ones(adj.shape[1], dtype=int)
    size = 0
    for root in range(n):
        seen = np.zeros(adj.shape[1], dtype=bool)
        stack, parent = [(root, 0)], {}
        found = -1
        while stack and found < 0:
            i, p = stack.pop()
            while p < len(nbrs[i]):
                j = nbrs[i][p]
                p += 1
                if seen[j]:
                    continue
                seen[j] = True
                parent[j] = i
                if owner[j] < 0:
                    found = j
                else:
                    stack.append((i, p))
                    stack.append((owner[j], 0))
                break
        if found < 0:
            continue
        j = found
        while True:  # flip the path back to the root
            i = parent[j]
            prev = np.nonzero(owner == i)[0]
            owner[j] = i
            if i == root:
                break
            j = prev[0]
        size += 1
    return size


def assign_spectrum(lam, ref, radius, use_scipy=True):
    """True if there is a one-to-one assignment of the computed eigenvalues lam to the reference eigenvalues ref with
    |lam_j - ref_i| <= radius_i: a perfect matching of the bipartite graph of the admissible pairs"""
    lam, ref = np.asarray(lam, dtype=complex).ravel(), np.asarray(ref, dtype=complex).ravel()
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), ref.shape)
    if lam.shape != ref.shape or not np.isfinite(lam).all():
        return False
    if lam.size == 0:
        return True
    adj = np.abs(ref[:, None] - lam[None, :]) <= radius[:, None]
    if not (adj.any(axis=0).all() and adj.any(axis=1).all()):
        return False
    linear_sum_assignment = None
    if use_scipy:
        try:
            from scipy.optimize import linear_sum_assignment
        except ImportError:
            pass
    if linear_sum_assignment is not None:
        cost = (~adj).astype(np.float64)
        r, c = linear_sum_assignment(cost)
        return bool(cost[r, c].sum() == 0)
    return _augmenting_paths(adj) == lam.size


def guard_sites(t, dtype):
    """The back substitution of eigvec_block (csrc/schur_core.h) on the quasi upper triangular t with standardised blocks, step
    for step in np.longdouble (exponents to 1e+-4932): the same starting components, the same divisor floor eps(dtype) |T|, but
    no rescaling, so nothing is lost and nothing overflows.  The guard of `dtype` is followed on the side: it fires where a new
    component, times the product of the earlier rescalings, passes the threshold.  Returns (largest component of any unscaled
    vector, the set of places where the guard fires, largest component of any vector after its rescalings); a place is
    (columns, pivot) with columns "real" or "pair" and pivot 1 or 2."""
    L, CL = np.longdouble, np.clongdouble
    t = np.asarray(t, dtype=np.float64).astype(L)
    n = t.shape[0]
    big = L(guard_threshold(dtype))
    floor = L(eps_of(dtype)) * np.abs(np.triu(t, -1)).sum()
    sub = np.concatenate([np.diag(t, -1) != 0, [False]])
    top, sites, out_top = L(0), set(), L(0)
    k = n - 1
    while k >= 0:
        pair = k > 0 and sub[k - 1]
        x = np.zeros(n, dtype=CL)
        if pair:
            q = np.sqrt(abs(t[k, k - 1])) * np.sqrt(abs(t[k - 1, k]))
            lam = CL(t[k, k]) + CL(1j) * CL(q)
            if abs(t[k - 1, k]) >= abs(t[k, k - 1]):
                x[k - 1], x[k] = 1, CL(1j) * CL(q / t[k - 1, k])
            else:
                x[k - 1], x[k] = CL(-q / t[k, k - 1]), CL(1j)
            i = k - 1
        else:
            lam = CL(t[k, k])
            x[k] = 1
            i = k
        rhs = -(t[:i, :].astype(CL) @ x)
        scale = L(1)
        while i > 0:
            i -= 1
            if i > 0 and sub[i - 1]:
                a, b, c = CL(t[i, i]) - lam, CL(t[i - 1, i]), CL(t[i, i - 1])
                det = a * a - b * c
                if pair and abs(det) < floor:
                    det = CL(floor)
                new = np.array([a * rhs[i - 1] - b * rhs[i], a * rhs[i] - c * rhs[i - 1]]) / det
                x[i - 1:i + 1] = new
                rhs[:i - 1] -= t[:i - 1, i - 1:i + 1].astype(CL) @ new
                mag, piv = max(abs(new[0].real), abs(new[0].imag), abs(new[1].real), abs(new[1].imag)), 2
                i -= 1
            else:
                z = CL(t[i, i]) - lam
                if abs(z) < floor:
                    z = CL(floor)
                x[i] = rhs[i] / z
                rhs[:i] -= t[:i, i].astype(CL) * x[i]
                mag, piv = max(abs(x[i].real), abs(x[i].imag)), 1
            if mag * scale > big:
                sites.add(("pair" if pair else "real", piv))
                scale = 1 / mag
        col = max(np.abs(x.real).max(), np.abs(x.imag).max())
        top, out_top = max(top, col), max(out_top, col * scale)
        k -= 2 if pair else 1
    return top, sites, out_top
