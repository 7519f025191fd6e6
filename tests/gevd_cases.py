"""Inputs and verdicts of the generalized EVD tests (tests/test_gpu_gevd.py on the GPU, tests/test_qz_host.py on the host build of
the same bodies, tests/test_gevd_cases.py for this module alone).  Pure numpy; scipy where it is installed, else the recorded
results of tests/golden/gevd_bounds.json and gevd_spectra.npz (written by tests/golden/make_gevd_bounds.py).

Verdicts, both invariant under any scaling of a column and of (alpha, beta):
  pair_residuals    |beta A x - alpha B x|_2 / ((|beta| |A|_F + |alpha| |B|_F) |x|_2) per column, and the same with
                    y^H (beta A - alpha B) for the left vectors.  Bound: 4 max(the reference solver's own value in the dtype of the
                    case, n eps), the rule of tests/evd_cases.py.
  assign_pairs      a one-to-one assignment of the computed (alpha, beta) to the reference's in the chordal metric, reference i
                    within c n eps kappa_i, kappa_i = |x_i| |y_i| sqrt(|A|_F^2 + |B|_F^2) / sqrt(|y_i^H A x_i|^2 + |y_i^H B x_i|^2) from
                    the reference's fp64 vectors, c as in evd_cases.reference_spectrum.  References whose radius exceeds 1 are left
                    out; at most 10 % of a case may be.  The matching is the one behind evd_cases.assign_spectrum (that function
                    takes points of the plane; the chordal metric is a metric of the sphere, so the adjacency is built here).

The reference solver is scipy.linalg.eig(a, b, left=True, right=True, homogeneous_eigvals=True).

Range cases (RANGE_SCALES): the `random` kind as (A 2^ka, B 2^kb), every scale an exact power of two, per dtype
  * apart and inside: |lambda| 2^(ka - kb) and its square are representable;
  * apart and beyond sqrt(max): lambda^2 (2^+-80, 2^+-120 in fp32; 2^+-600, 2^+-960 in fp64) is not, and at +-60 / +-480 lambda
    itself is not: only the pair (alpha, beta) can carry it;
  * common: both matrices at one end of the range.
The rows are the largest the issue of these tests names; range_representable (the counterpart of range_cases.cap_ok) holds at
every one of them and every size the tests use, inputs and expected (alpha 2^ka, beta 2^kb) alike, so none had to be shrunk.
The verdicts run on unscaled quantities (range_check): alpha 2^-ka and beta 2^-kb are exact, the eigenvectors are scale-free, so
the recorded reference of `random` and its bounds apply unchanged."""
import json
import os

import numpy as np

import evd_cases as ec

try:
    import scipy.linalg as _sla
except ImportError:  # the recorded results take its place
    _sla = None

DTYPES = [np.float64, np.float32]
KINDS = ["random", "identity_b", "triangular_pair", "symmetric_definite", "rotation_blocks", "singular_b1", "singular_bq", "graded", "scaled"]
HOST_SIZES = [1, 2, 3, 15, 16, 17, 35]
# kinds built for the eigenvector stage (gevec_block of csrc/qz_core.h): triangular pairs with a nonnegative diagonal of B, which
# stage 2 leaves as they are (zero sweeps; alpha and beta are the diagonals), and their rotations Q A Z^T, Q B Z^T, which reach the
# same substitution behind real sweeps.  They run at sizes of their own (vector_cases), not at the sizes of KINDS.
TRIANGLE_KINDS = ["graded_triangular_pair", "jordan_pair", "infinite_in_triangle"]
VECTOR_KINDS = TRIANGLE_KINDS + ["rotated_" + k for k in TRIANGLE_KINDS]
# kinds under the residual verdict alone (the precedent of evd_cases.DEFECTIVE and its rotated kinds).  jordan_pair is defective.
# graded_triangular_pair: a component beyond 1 / sqrt(min positive) ~ 1e154 next to a starting component 1 means that
# beta_k A - alpha_k B, entries of order one, has a leading block whose inverse is that large, so the eigenvalue condition numbers
# are of that order too and every radius c n eps kappa_i exceeds the chordal diameter 1: the cap of 10 % left out and a guard that
# fires exclude each other.  Its eigenvalues are checked exactly instead (alpha, beta are the diagonals, bit for bit).
RESIDUAL_ONLY = {"graded_triangular_pair", "jordan_pair"} | {"rotated_" + k for k in TRIANGLE_KINDS}
# rows of graded_triangular_pair: the smallest count at which the guard of fp64 fires (pair_guard_replay; one leaf of either dtype)
GUARD_N = 37
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gevd_bounds.json")  # the residuals, one line per case
GOLDEN_SPECTRA = os.path.join(os.path.dirname(GOLDEN), "gevd_spectra.npz")  # alpha, beta, kappa of every case: binary, not text
SCALE_K = 10
# exponents of D1 and of D2 in `graded`, per side.  fp64: the entries of D1 X D2 span 2^+-20.  fp32: kappa_i grows by up to
# 2^(4 span) and the assignment leaves out every pair with c n eps kappa_i > 1, that is kappa_i > 2^13 at n = 293; with more than
# +-1 per side the reference solver itself leaves out more than the 10 % the verdict allows
GRADED_SPAN = {np.dtype(np.float64): 10, np.dtype(np.float32): 1}
# a seed is replaced where the reference solver does not pass its own verdicts on the case (tests/test_gevd_cases.py)
SEEDS = {}


def infinite_rows(n):
    """rows of the exact zeros on diag(B) in infinite_in_triangle"""
    return sorted({0, n // 2, n - 1})


def vector_cases(sizes):
    return [(kind, n) for kind in VECTOR_KINDS for n in sizes if exists(kind, n)]


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def singular_count(kind, n):
    """zero columns of B in the singular kinds; 0: the case does not exist at this n"""
    if kind == "singular_b1":
        return 1
    return n // 4 if n // 4 > 1 else 0


def exists(kind, n):
    if kind.endswith("infinite_in_triangle"):
        # the three zeros of diag(B) make one defective infinite eigenvalue (B loses less rank than its diagonal shows): its three
        # references have no finite condition number and are left out of the assignment, which allows 10 % of n
        return n >= 30
    return not kind.startswith("singular_b") or singular_count(kind, n) > 0


def _orth(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


def generate(kind, n, dtype, seed=None):
    """(A, B) of the case in `dtype`"""
    if seed is None:
        seed = SEEDS.get((kind, n, np.dtype(dtype).name), 0)
    if kind.startswith("rotated_"):
        rng = np.random.default_rng(100000 * (KINDS + VECTOR_KINDS).index(kind) + 1000 * seed + n)
        a, b = generate(kind[len("rotated_"):], n, dtype, seed)
        q, z = _orth(rng, n), _orth(rng, n)
        return np.asarray(q @ a.astype(np.float64) @ z.T, dtype=dtype), np.asarray(q @ b.astype(np.float64) @ z.T, dtype=dtype)
    rng = np.random.default_rng(100000 * (KINDS + VECTOR_KINDS).index(kind) + 1000 * seed + n)
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    if kind == "random":
        pass
    elif kind == "identity_b":
        b = np.eye(n)
    elif kind == "triangular_pair":
        # (random triangular matrices are far from normal: the strict parts are damped and the eigenvalues kept apart, so that
        # the condition numbers stay moderate at every size)
        a, b = np.triu(a, 1) / (2 * np.sqrt(n)), np.triu(b, 1) / (2 * np.sqrt(n))
        idx = np.arange(n)
        a[idx, idx] = rng.permutation(1.0 + idx) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        b[idx, idx] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (1.0 + rng.random(n))
    elif kind == "symmetric_definite":
        a = a + a.T
        b = b @ b.T + n * np.eye(n)
    elif kind == "rotation_blocks":
        da = np.zeros((n, n))
        for i in range(0, n - 1, 2):
            r, th = 0.5 + rng.random(), 0.3 + 2.5 * rng.random()
            da[i:i + 2, i:i + 2] = r * np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]])
        if n % 2:
            da[n - 1, n - 1] = 1.0 + rng.random()
        q, z = _orth(rng, n), _orth(rng, n)
        a, b = q @ da @ z.T, q @ z.T
    elif kind.startswith("singular_b"):
        k = singular_count(kind, n)
        cols = np.sort(rng.choice(n, size=k, replace=False))
        b[:, cols] = 0.0
        b = _orth(rng, n) @ b
        b[:, cols] = 0.0  # (a product with exact zeros is exactly zero; kept explicit)
    elif kind == "graded":
        span = GRADED_SPAN[np.dtype(dtype)]
        k1, k2 = rng.integers(-span, span + 1, n), rng.integers(-span, span + 1, n)
        if n > 1:
            k1[0], k1[-1], k2[0], k2[-1] = -span, span, span, -span
        a = np.ldexp(np.ldexp(np.asarray(a, dtype=dtype).astype(np.float64), k1[:, None]), k2[None, :])
        b = np.ldexp(np.ldexp(np.asarray(b, dtype=dtype).astype(np.float64), k1[:, None]), k2[None, :])
    elif kind == "scaled":
        a, b = generate("random", n, dtype)
        return np.ldexp(a, SCALE_K), np.ldexp(b, -SCALE_K)
    elif kind == "graded_triangular_pair":
        # diag(B) = 1, 2, 1, 2, ...; diag(A) / diag(B) = 1 + i 1e-3, distinct in either dtype; 1e3 on the first two superdiagonals
        # of A and 5e2 on the first of B: a vector grows by about 1e6 / j at the j-th row above its own
        idx = np.arange(n)
        db = 1.0 + (idx % 2)
        a = np.diag(np.asarray(1.0 + 1e-3 * idx, dtype=dtype).astype(np.float64) * db)
        b = np.diag(db)
        for d in (1, 2):
            a += np.diag(np.full(n - d, 1e3), d) if n > d else 0
        b += np.diag(np.full(n - 1, 5e2), 1) if n > 1 else 0
    elif kind == "jordan_pair":
        a, b = 2.0 * np.eye(n) + np.diag(np.ones(n - 1), 1), np.eye(n)
    elif kind == "infinite_in_triangle":
        # triangular_pair with diag(B) > 0 and exact zeros on it at the top, in the interior and at the bottom
        a, b = np.triu(a, 1) / (2 * np.sqrt(n)), np.triu(b, 1) / (2 * np.sqrt(n))
        idx = np.arange(n)
        a[idx, idx] = rng.permutation(1.0 + idx) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        b[idx, idx] = 1.0 + rng.random(n)
        b[infinite_rows(n), infinite_rows(n)] = 0.0
    else:
        raise ValueError(kind)
    return np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)


def unpack(alpha, alpha_im, beta, u):
    """complex alpha and eigenvector columns from the packed layout; asserts the pair layout of alpha_im"""
    n = alpha.shape[0]
    al = alpha.astype(np.float64) + 1j * alpha_im.astype(np.float64)
    V = None if u is None else np.zeros((n, n), complex)
    i = 0
    while i < n:
        if alpha_im[i] == 0:
            if u is not None:
                V[:, i] = u[:, i]
            i += 1
        else:
            assert i + 1 < n and alpha_im[i] > 0 and alpha_im[i + 1] == -alpha_im[i], f"alpha_im does not hold a pair at {i}"
            if u is not None:
                V[:, i] = u[:, i].astype(np.float64) + 1j * u[:, i + 1].astype(np.float64)
                V[:, i + 1] = V[:, i].conj()
            i += 2
    return al, V


def _exponent(x):
    """e with 2^(e - 1) <= max |x| < 2^e; 0 for a zero or non-finite matrix"""
    m = np.abs(x).max(initial=0.0)
    return int(np.frexp(m)[1]) if np.isfinite(m) and m > 0 else 0


def _ldexp(x, e):
    """x 2^e, in two exact steps (2^e alone need not be representable)"""
    return x * 2.0 ** (e // 2) * 2.0 ** (e - e // 2)


def pair_residuals(a, b, alpha, beta, V, side="right"):
    """per column, in fp64, every column divided by its largest entry first and (alpha, beta) by its larger modulus; a zero or
    non-finite column has the residual inf.  A and B may lie anywhere in the range of fp64, each on a scale of its own."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    V = np.asarray(V, dtype=complex)
    alpha, beta = np.asarray(alpha, dtype=complex), np.asarray(beta, dtype=complex)
    # A and alpha by one power of two, B and beta by another, so that |A| and |B| are of order one: beta A - alpha B is only
    # multiplied by their product, the quotient is unchanged, and no square below (np.linalg.norm) can leave the range
    ea, eb = _exponent(a64), _exponent(b64)
    a64, alpha, b64, beta = _ldexp(a64, -ea), _ldexp(alpha, -ea), _ldexp(b64, -eb), _ldexp(beta, -eb)
    m = np.maximum(np.abs(alpha), np.abs(beta))
    big = np.abs(V).max(axis=0) if V.size else np.zeros(0)
    bad = ~np.isfinite(big) | (big == 0) | ~np.isfinite(m) | (m == 0)
    Vs = np.where(bad[None, :], 0.0, V) / np.where(bad, 1.0, big)[None, :]
    al, be = np.where(bad, 0, alpha) / np.where(bad, 1.0, m), np.where(bad, 0, beta) / np.where(bad, 1.0, m)
    if side == "right":
        r = (a64 @ Vs) * be - (b64 @ Vs) * al
    else:  # (y^H (beta A - alpha B))^H = conj(beta) A^T y - conj(alpha) B^T y
        r = (a64.T @ Vs) * be.conj() - (b64.T @ Vs) * al.conj()
    den = (np.abs(be) * np.linalg.norm(a64) + np.abs(al) * np.linalg.norm(b64)) * np.where(bad, 1.0, np.linalg.norm(Vs, axis=0))
    return np.where(bad, np.inf, np.linalg.norm(r, axis=0) / np.maximum(den, 1e-300))


def chordal(al1, be1, al2, be2):
    """matrix of chordal distances |a1 b2 - a2 b1| / (|(a1, b1)| |(a2, b2)|)"""
    al1, be1, al2, be2 = (np.asarray(v, dtype=complex) for v in (al1, be1, al2, be2))
    n1, n2 = np.sqrt(np.abs(al1) ** 2 + np.abs(be1) ** 2), np.sqrt(np.abs(al2) ** 2 + np.abs(be2) ** 2)
    s1, s2 = np.where(n1 > 0, n1, 1.0), np.where(n2 > 0, n2, 1.0)
    return np.abs((al1 / s1)[:, None] * (be2 / s2)[None, :] - (al2 / s2)[None, :] * (be1 / s1)[:, None])


def assign_pairs(alpha, beta, ref):
    """(ok, references left out): every reference pair within its radius of a computed pair of its own"""
    al, be = np.asarray(alpha, dtype=complex), np.asarray(beta, dtype=complex)
    if al.shape != ref["alpha"].shape or not (np.isfinite(al).all() and np.isfinite(be).all()):
        return False, 0
    keep = ref["radius"] <= 1.0
    left_out = int((~keep).sum())
    if left_out > 0.1 * al.size:
        return False, left_out
    adj = chordal(ref["alpha"][keep], ref["beta"][keep], al, be) <= ref["radius"][keep][:, None]
    if adj.shape[0] == 0:
        return True, left_out
    if not adj.any(axis=1).all():
        return False, left_out
    return ec._augmenting_paths(adj) == adj.shape[0], left_out


def _solve(a, b):
    """the reference solver: (alpha, beta, right vectors, left vectors)"""
    w, vl, vr = _sla.eig(a, b, left=True, right=True, homogeneous_eigvals=True)
    return w[0].astype(complex), w[1].astype(complex), vr.astype(complex), vl.astype(complex)


def _compute(kind, n, dtype):
    a, b = generate(kind, n, dtype)
    e = eps_of(dtype)
    al, be, vr, vl = _solve(a, b)
    res_r = float(pair_residuals(a, b, al, be, vr).max(initial=0.0))
    res_l = float(pair_residuals(a, b, al, be, vl, "left").max(initial=0.0))
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    al64, be64, x, y = _solve(a64, b64)
    ya, yb = np.einsum("ij,ij->j", y.conj(), a64 @ x), np.einsum("ij,ij->j", y.conj(), b64 @ x)
    with np.errstate(all="ignore"):
        kappa = (np.linalg.norm(x, axis=0) * np.linalg.norm(y, axis=0) * np.sqrt(np.linalg.norm(a64) ** 2 + np.linalg.norm(b64) ** 2)
                 / np.sqrt(np.abs(ya) ** 2 + np.abs(yb) ** 2))
    kappa = np.where(np.isfinite(kappa), np.maximum(kappa, 1.0), np.inf)
    return {"res_right": res_r, "res_left": res_l, "alpha": al64, "beta": be64, "kappa": kappa, "own_alpha": al, "own_beta": be}


def _key(kind, n, dtype):
    return f"{kind}/{n}/{np.dtype(dtype).name}/{SEEDS.get((kind, n, np.dtype(dtype).name), 0)}"


def encode(rec):
    """one record as the golden files keep it: (the scalars of gevd_bounds.json, the arrays of gevd_spectra.npz)"""
    return ({"res_right": rec["res_right"], "res_left": rec["res_left"]},
            {"alpha": np.asarray(rec["alpha"], dtype=np.complex128), "beta": np.asarray(rec["beta"].real, dtype=np.float64),
             "kappa": np.minimum(rec["kappa"], 3e38).astype(np.float32)})


def spectra_offsets(keys):
    """{key: first index of the case in the arrays of gevd_spectra.npz}; a key is kind/n/dtype/seed"""
    out, lo = {}, 0
    for k in sorted(keys):
        out[k] = lo
        lo += int(k.split("/")[1])
    return out


_GOLDEN = None
_CACHE = {}


def reference(kind, n, dtype, prefer_golden=False):
    """{"res_right", "res_left", "alpha", "beta", "kappa", "radius"} of the case, once per case"""
    global _GOLDEN
    key = _key(kind, n, dtype)
    if (key, prefer_golden) in _CACHE:
        return _CACHE[(key, prefer_golden)]
    if _sla is not None and not prefer_golden:
        rec = _compute(kind, n, dtype)
    else:
        if _GOLDEN is None:
            _GOLDEN = (json.load(open(GOLDEN)), np.load(GOLDEN_SPECTRA))
        g, z = _GOLDEN[0][key], _GOLDEN[1]
        lo = spectra_offsets(_GOLDEN[0])[key]  # the arrays of all cases, end to end in the order of the sorted keys
        rec = {"res_right": g["res_right"], "res_left": g["res_left"], "alpha": z["alpha"][lo:lo + n],
               "beta": z["beta"][lo:lo + n].astype(complex), "kappa": z["kappa"][lo:lo + n].astype(np.float64)}
    c = 8.0 if np.dtype(dtype) == np.float64 else 4.0
    rec["radius"] = c * n * eps_of(dtype) * rec["kappa"]
    _CACHE[(key, prefer_golden)] = rec
    return rec


def bounds(kind, n, dtype):
    """(right bound, left bound): 4 max(the reference's own value in the dtype of the case, n eps)"""
    r = reference(kind, n, dtype)
    return 4 * max(r["res_right"], n * eps_of(dtype)), 4 * max(r["res_left"], n * eps_of(dtype))


def check(kind, n, dtype, a, b, alpha, alpha_im, beta, ur=None, ul=None, verbose=True, stage0_identity=True):
    """both verdicts and the expectations of the kind on one result; raises AssertionError.  stage0_identity=False: the QR of B
    that came first is not the identity on this triangular pair (a zero column does not advance the row of the next reflector, in
    the reference as in csrc/qr.hip, so a singular triangular B comes back as another triangle): the diagonals are not expected"""
    ref = reference(kind, n, dtype)
    assert np.isfinite(alpha).all() and np.isfinite(alpha_im).all() and np.isfinite(beta).all()
    al, VR = unpack(alpha, alpha_im, beta, ur)
    _, VL = unpack(alpha, alpha_im, beta, ul)
    be = beta.astype(np.float64)
    br, bl = bounds(kind, n, dtype)
    for V, side, bound in ((VR, "right", br), (VL, "left", bl)):
        if V is None:
            continue
        res = pair_residuals(a, b, al, be, V, side)
        if verbose:
            print(f"{kind} n={n} {np.dtype(dtype).name} {side}: worst residual {res.max(initial=0.0):.3e} bound {bound:.3e}")
        assert res.max(initial=0.0) <= bound, (kind, n, side, float(res.max()), bound, int(res.argmax()))
    if kind == "infinite_in_triangle" and not stage0_identity:
        k = len(infinite_rows(n))
        assert (alpha_im == 0).all() and int((beta == 0).sum()) == k and int((beta > 0).sum()) == n - k, (kind, n, int((beta == 0).sum()))
    elif kind in TRIANGLE_KINDS:  # stage 2 leaves a triangular pair with a nonnegative diag(B) as it is
        da, db = np.diag(a), np.diag(b)
        assert (alpha_im == 0).all() and np.array_equal(beta, db), (kind, n, "beta is not diag(B)", np.nonzero(beta != db)[0], beta[beta != db], db[beta != db])
        assert np.array_equal(np.abs(alpha), np.abs(da)) and np.array_equal(alpha[db > 0], da[db > 0]), (kind, n, "alpha is not diag(A)")
        if kind == "infinite_in_triangle":
            assert np.array_equal(np.nonzero(beta == 0)[0], infinite_rows(n)) and (np.delete(beta, infinite_rows(n)) > 0).all()
    if kind in RESIDUAL_ONLY:
        return
    ok, left_out = assign_pairs(al, be, ref)
    if verbose:
        print(f"{kind} n={n} {np.dtype(dtype).name}: assignment {ok}, {left_out} left out")
    assert ok, (kind, n, "spectrum assignment", left_out)
    if kind == "symmetric_definite":
        if not (alpha_im == 0).all():  # each imaginary part within the radius of the reference pair nearest to its own
            d = chordal(ref["alpha"], ref["beta"], al, beta.astype(np.float64))
            own = ref["radius"][d.argmin(axis=0)]
            assert (np.abs(alpha_im) / np.maximum(np.hypot(np.abs(al), np.abs(beta)), 1e-300) <= own).all()
    if kind == "rotation_blocks":
        assert int((alpha_im > 0).sum()) == n // 2 and int((alpha_im < 0).sum()) == n // 2  # (unpack has checked that pairs are adjacent)
    if kind.startswith("singular_b"):
        k = singular_count(kind, n)
        assert int((beta == 0).sum()) == k and int((np.abs(beta) > 0).sum()) == n - k, (kind, n, int((beta == 0).sum()))


# ---- the ends of the range: (ka, kb) of A 2^ka, B 2^kb on the `random` kind
RANGE_SCALES = {
    np.dtype(np.float32): {"inside": [(20, -20), (-20, 20)], "beyond": [(40, -40), (-40, 40), (60, -60), (-60, 60)], "common": [(60, 60), (-60, -60)]},
    np.dtype(np.float64): {"inside": [(100, -100), (-100, 100)], "beyond": [(300, -300), (-300, 300), (480, -480), (-480, 480)],
                           "common": [(480, 480), (-480, -480)]},
}
RANGE_HOST_SIZES = [15, 17, 35]  # with edge 16: one leaf, the smallest block that takes windows, several windows


def range_rows(dtype):
    """[(group, ka, kb)] of the dtype"""
    return [(group, ka, kb) for group, rows in RANGE_SCALES[np.dtype(dtype)].items() for ka, kb in rows]


def cap_ok(x):
    """every entry finite and either exactly zero or a normal number of x's dtype (range_cases.cap_ok)"""
    x = np.asarray(x)
    assert x.dtype in (np.dtype(np.float64), np.dtype(np.float32))
    ax = np.abs(x)
    return bool(np.isfinite(x).all() and ((ax == 0) | (ax >= np.finfo(x.dtype).tiny)).all())


def range_generate(n, dtype, ka, kb):
    """(A, B) of `random` and (A 2^ka, B 2^kb), all in `dtype`"""
    a, b = generate("random", n, dtype)
    return a, b, np.ldexp(a, ka), np.ldexp(b, kb)


def range_representable(n, dtype, ka, kb):
    """the scaled inputs and the expected alpha 2^ka, beta 2^kb (the reference's spectrum in `dtype`) are finite and normal, and
    scaling them back is exact"""
    a, b, sa, sb = range_generate(n, dtype, ka, kb)
    ref = reference("random", n, dtype)
    al_re, al_im, be = (np.asarray(v, dtype=dtype) for v in (ref["alpha"].real, ref["alpha"].imag, ref["beta"].real))
    parts = [(a, sa, ka), (b, sb, kb), (al_re, np.ldexp(al_re, ka), ka), (al_im, np.ldexp(al_im, ka), ka), (be, np.ldexp(be, kb), kb)]
    return all(x.dtype == np.dtype(dtype) and cap_ok(x) and np.array_equal(np.ldexp(x, -k), x0) for x0, x, k in parts)


def range_check(n, dtype, ka, kb, alpha, alpha_im, beta, ur=None, ul=None, verbose=True):
    """both verdicts of `random` on the result of (A 2^ka, B 2^kb), on unscaled quantities"""
    a, b, _, _ = range_generate(n, dtype, ka, kb)
    for x in (alpha, alpha_im, beta):
        assert x.dtype == np.dtype(dtype) and np.isfinite(x).all()
    if verbose:
        print(f"random n={n} {np.dtype(dtype).name} as (A 2^{ka}, B 2^{kb}), unscaled:")
    check("random", n, dtype, a, b, np.ldexp(alpha, -ka), np.ldexp(alpha_im, -ka), np.ldexp(beta, -kb), ur, ul, verbose)


def guard_threshold(dtype):
    """1 / sqrt(min positive): gevec_block rescales a vector when a new component passes it"""
    return 1.0 / float(np.sqrt(np.float64(np.finfo(dtype).tiny)))


def pair_guard_replay(a, b, dtype):
    """The back substitution of gevec_block (csrc/qz_core.h) for the right vectors of a triangular pair with real eigenvalues,
    step for step in np.longdouble (exponents to 1e+-4932): the same (acoef, bcoef) from ascale, bscale, the same pivot floor
    dmin, but no rescaling, so nothing is lost and nothing overflows.  The guard of `dtype` is followed on the side: it fires
    where a new component, times the product of the earlier rescalings, passes the threshold.  Returns (largest component of any
    unscaled vector, times the guard fires, divisors replaced by the floor, divisors in all)."""
    L = np.longdouble
    S, P = np.asarray(a, dtype=dtype).astype(L), np.asarray(b, dtype=dtype).astype(L)
    n = S.shape[0]
    assert (np.tril(S, -1) == 0).all() and (np.tril(P, -1) == 0).all()
    e, tiny, big = L(eps_of(dtype)), L(np.finfo(dtype).tiny), L(guard_threshold(dtype))
    snorm, pnorm = np.sqrt((S * S).sum()), np.sqrt((P * P).sum())
    ascale, bscale = 1 / max(snorm, tiny), 1 / max(pnorm, tiny)
    top, fired, floored, divisors = L(0), 0, 0, 0
    for k in range(n):
        alr, bet = S[k, k], P[k, k]
        temp = 1 / max(abs(alr) * ascale, abs(bet) * bscale, tiny)
        acoef, bcoef = ((temp * bet) * bscale) * ascale, ((temp * alr) * ascale) * bscale
        dmin = max(e * abs(acoef) * snorm, e * abs(bcoef) * pnorm, tiny)
        M = acoef * S - bcoef * P
        x = np.zeros(n, dtype=L)
        x[k] = 1
        rhs = -M[:k, k].copy()
        scale = L(1)
        for i in range(k - 1, -1, -1):
            d = M[i, i]
            divisors += 1
            if abs(d) < dmin:
                d, floored = dmin, floored + 1
            x[i] = rhs[i] / d if rhs[i] != 0 else 0
            if abs(x[i]) * scale > big:
                fired += 1
                scale = 1 / abs(x[i])
            rhs[:i] -= M[:i, i] * x[i]
        top = max(top, np.abs(x).max())
    return top, fired, floored, divisors


def all_cases(sizes):
    return [(kind, n) for kind in KINDS for n in sizes if exists(kind, n)]
