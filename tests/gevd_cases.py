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

The reference solver is scipy.linalg.eig(a, b, left=True, right=True, homogeneous_eigvals=True)."""
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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gevd_bounds.json")  # the residuals, one line per case
GOLDEN_SPECTRA = os.path.join(os.path.dirname(GOLDEN), "gevd_spectra.npz")  # alpha, beta, kappa of every case: binary, not text
SCALE_K = 10
# exponents of D1 and of D2 in `graded`, per side.  fp64: the entries of D1 X D2 span 2^+-20.  fp32: kappa_i grows by up to
# 2^(4 span) and the assignment leaves out every pair with c n eps kappa_i > 1, that is kappa_i > 2^13 at n = 293; with more than
# +-1 per side the reference solver itself leaves out more than the 10 % the verdict allows
GRADED_SPAN = {np.dtype(np.float64): 10, np.dtype(np.float32): 1}
# a seed is replaced where the reference solver does not pass its own verdicts on the case (tests/test_gevd_cases.py)
SEEDS = {}


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def singular_count(kind, n):
    """zero columns of B in the singular kinds; 0: the case does not exist at this n"""
    if kind == "singular_b1":
        return 1
    return n // 4 if n // 4 > 1 else 0


def exists(kind, n):
    return not kind.startswith("singular_b") or singular_count(kind, n) > 0


def _orth(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


def generate(kind, n, dtype, seed=None):
    """(A, B) of the case in `dtype`"""
    if seed is None:
        seed = SEEDS.get((kind, n, np.dtype(dtype).name), 0)
    rng = np.random.default_rng(100000 * KINDS.index(kind) + 1000 * seed + n)
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


def pair_residuals(a, b, alpha, beta, V, side="right"):
    """per column, in fp64, every column divided by its largest entry first and (alpha, beta) by its larger modulus; a zero or
    non-finite column has the residual inf"""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    V = np.asarray(V, dtype=complex)
    alpha, beta = np.asarray(alpha, dtype=complex), np.asarray(beta, dtype=complex)
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


def check(kind, n, dtype, a, b, alpha, alpha_im, beta, ur=None, ul=None, verbose=True):
    """both verdicts and the expectations of the kind on one result; raises AssertionError"""
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


def all_cases(sizes):
    return [(kind, n) for kind in KINDS for n in sizes if exists(kind, n)]
