"""General real EVD on the GPU (include/faer_hip.h section 2i, csrc/schur.hip): every size at which the Schur driver takes another
path (one leaf for n <= W, window sweeps above, W the window edge of the dtype), six kinds of input, the failure paths, and the
project's standing families (host operands, padded / offset / transposed views, a non-blocking caller stream, the ends of the
floating-point range, a poisoned scratch pool).

Bound.  For every input numpy's eig (LAPACK geev in the same dtype) is run on the CPU on the same matrix and its residual
r_np = |A V - V L|_F / (|A|_F |V|_F) measured; the bound of the case is 4 max(r_np, n eps).  The factor 4 allows for a
different shift sequence and the missing early deflation, both backward stable at the same order.  Measured r_np (in units of
eps of the dtype) on the inputs of this file: float64, N(0,1): 0.5 (n = 2), 2.3 (3), 2.1 (95), 2.2 (96), 2.0 (97), 2.1 (195), 1.8
(337); symmetric 1.4 .. 1.8, triangular 0 .. 0.2, block diagonal 0 .. 1.8, cyclic 1.4 .. 2.9, normal 0.1 .. 1.8.  float32: at most
0.2 for every kind and size (numpy's eig of a float32 matrix rounds a double-precision result).  All are below n eps from n = 3
on, so the bound in force is 4 n eps (n = 2: 8 eps, n = 1: 4 eps; the code's residuals there were 0.6 and 0)."""
import ctypes as C

import numpy as np
import pytest

import range_cases as RC
from gpu_util import EPS, guard_intact, init_gpu, ordered_call, place, same_result, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
WEDGE = {np.dtype(np.float64): 96, np.dtype(np.float32): 128}


def sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [1, 2, 3, W - 1, W, W + 1, 2 * W + 3, {96: 337, 128: 449}[W]]


def make(kind, n, dtype, seed=0):
    """(matrix, known eigenvalues or None)"""
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


KINDS = ["normal01", "symmetric", "triangular", "block_diagonal", "cyclic", "normal"]
_BOUNDS = {}


def bound(a, key):
    """4 max(residual of numpy's eig in the dtype of a, n eps), computed once per input"""
    if key not in _BOUNDS:
        n = a.shape[0]
        w, v = np.linalg.eig(a)
        a64 = a.astype(np.float64)
        r = np.linalg.norm(a64 @ v - v * w) / max(np.linalg.norm(a64) * np.linalg.norm(v), 1e-300)
        e = float(EPS[a.dtype])
        print(f"numpy eig residual {key}: {r / e:.2f} eps (n eps = {n} eps)")
        _BOUNDS[key] = 4 * max(r, n * e)
    return _BOUNDS[key]


def run(F, a, left=True, right=True, order="F"):
    import torch

    n = a.shape[0]
    tdt = torch.float64 if a.dtype == np.float64 else torch.float32
    da = to_dev(a, order)
    s = torch.full((n,), -7.5, dtype=tdt, device="cuda")
    si = torch.full((n,), -7.5, dtype=tdt, device="cuda")
    ul = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if left else None
    ur = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if right else None
    tag = F.evd(da, s, si, ul, ur)
    F.synchronize()
    assert np.array_equal(to_host(da), a, equal_nan=True), "A was written"
    return tag, s.cpu().numpy(), si.cpu().numpy(), (ul.cpu().numpy() if left else None), (ur.cpu().numpy() if right else None)


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


def check_vectors(a, s, si, ul, ur, b, what):
    a64 = a.astype(np.float64)
    na = max(np.linalg.norm(a64), 1e-300)
    lam = None
    for side, u in (("right", ur), ("left", ul)):
        if u is None:
            continue
        assert np.isfinite(u).all(), (what, side)
        lam, V = unpack(s, si, u)
        assert (np.abs(V).max(axis=0) > 0).all(), (what, side, "a zero eigenvector column")
        if side == "right":
            r = np.linalg.norm(a64 @ V - V * lam) / (na * np.linalg.norm(V))
        else:
            r = np.linalg.norm(V.conj().T @ a64 - lam[:, None] * V.conj().T) / (na * np.linalg.norm(V))
        print(f"{what} {side} residual {r / float(EPS[a.dtype]):.2f} eps, bound {b / float(EPS[a.dtype]):.0f} eps")
        assert r <= b, (what, side, r, b)
    if lam is None:
        lam, _ = unpack(s, si, None)
    return lam


def match(x, y):
    """largest distance from an entry of x to the nearest entry of y"""
    return np.abs(x[:, None] - y[None, :]).min(axis=1).max(initial=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_evd_kinds_and_sizes(kind, dtype):
    F = init_gpu()
    assert F.evd_window_edge(dtype) == WEDGE[np.dtype(dtype)]
    for n in sizes(dtype):
        a, known = make(kind, n, dtype)
        what = f"{kind} n={n} {np.dtype(dtype).name}"
        b = bound(a, (kind, n, np.dtype(dtype).name))
        tag, s, si, ul, ur = run(F, a)
        assert tag == F.EVD_OK, what
        print(what, F.debug_evd_last_counts())
        lam = check_vectors(a, s, si, ul, ur, b, what)
        na = np.linalg.norm(a.astype(np.float64))
        if kind == "symmetric":
            assert (si == 0).all(), what
            ref = np.linalg.eigvalsh(a.astype(np.float64))
            assert np.abs(np.sort(s.astype(np.float64)) - ref).max() <= b * na, what
        if kind == "triangular":
            assert (si == 0).all() and np.array_equal(np.sort(s), np.sort(np.diag(a))), what
        if known is not None:
            d = match(lam, known)
            assert d <= b * na, (what, d, b * na)
            assert lam.shape == known.shape and match(known, lam) <= b * na, what
        if kind == "normal01":
            # eigenvalues only: the same Schur form, so the same values up to the bound; each vector set alone
            tag0, s0, si0, _, _ = run(F, a, left=False, right=False)
            assert tag0 == F.EVD_OK
            lam0, _ = unpack(s0, si0, None)
            assert match(lam0, lam) <= b * na and match(lam, lam0) <= b * na, what
            tagl, sl, sil, ull, _ = run(F, a, left=True, right=False)
            tagr, sr, sir, _, urr = run(F, a, left=False, right=True)
            assert tagl == F.EVD_OK and tagr == F.EVD_OK
            check_vectors(a, sl, sil, ull, None, b, what + " UL only")
            check_vectors(a, sr, sir, None, urr, b, what + " UR only")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_no_convergence(bad, dtype):
    F = init_gpu()
    for n in (1, 5, WEDGE[np.dtype(dtype)] + 1):
        a, _ = make("normal01", n, dtype)
        a[n // 2, n // 3] = bad
        tag, _, _, _, _ = run(F, a)
        assert tag == F.EVD_NO_CONVERGENCE
    # and the next call is clean
    a, _ = make("normal01", 40, dtype)
    tag, s, si, ul, ur = run(F, a)
    assert tag == F.EVD_OK
    check_vectors(a, s, si, ul, ur, bound(a, ("normal01", 40, np.dtype(dtype).name)), "after a failure")


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_matrix(dtype):
    import torch

    F = init_gpu()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    a = torch.empty((0, 0), dtype=tdt, device="cuda")
    s = torch.empty((0,), dtype=tdt, device="cuda")
    assert F.evd(a, s, s.clone(), a.clone(), a.clone()) == F.EVD_OK
    assert F.evd(np.empty((0, 0), dtype=dtype), np.empty(0, dtype=dtype), np.empty(0, dtype=dtype)) == F.EVD_OK


def family_sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [W + 1, 2 * W + 3]


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_operands(dtype):
    F = init_gpu()
    for n in family_sizes(dtype):
        a, _ = make("normal01", n, dtype)
        b = bound(a, ("normal01", n, np.dtype(dtype).name))
        _, sd, sid, uld, urd = run(F, a)
        # a faer::Mat (column major), a row-major matrix and a strided view with strided S: the same values as device operands
        for layout in ("F", "C", "strided"):
            if layout == "strided":
                parent = np.full((2 * n + 3, n + 5), -7.5, dtype=dtype)
                parent[1:2 * n + 1:2, 2:n + 2] = a
                ha = parent[1:2 * n + 1:2, 2:n + 2]
            else:
                ha = np.array(a, order=layout)
            keep = ha.copy()
            sp, sip = np.full(2 * n, -7.5, dtype=dtype), np.full(n, -7.5, dtype=dtype)
            s, si = sp[::2], sip
            ul = np.full((n, n), -7.5, dtype=dtype, order="F")
            urp = np.full((n + 3, n + 2), -7.5, dtype=dtype, order="C")
            ur = urp[2:n + 2, 1:n + 1]
            assert F.evd(ha, s, si, ul, ur) == F.EVD_OK
            assert np.array_equal(ha, keep) and (sp[1::2] == -7.5).all()
            assert (urp[:2] == -7.5).all() and (urp[n + 2:] == -7.5).all() and (urp[:, 0] == -7.5).all() and (urp[:, n + 1:] == -7.5).all()
            if layout == "strided":
                assert (parent[0::2] == -7.5).all() and (parent[:, :2] == -7.5).all() and (parent[:, n + 2:] == -7.5).all()
            assert np.array_equal(s, sd) and np.array_equal(si, sid) and np.array_equal(ul, uld) and np.array_equal(ur, urd), (n, layout)
            check_vectors(a, s, si, ul, ur, b, f"host {layout} n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["sub", "rowpad", "mat"])
def test_device_views(layout, dtype):
    """padded and offset device views of every operand (tests/gpu_util.py layouts) and a transposed (row-major) A: the guard cells
    stay intact and the values are those of plain operands"""
    import torch

    F = init_gpu()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for n in family_sizes(dtype):
        a, _ = make("normal01", n, dtype)
        _, sd, sid, uld, urd = run(F, a)
        out0 = np.full((n, n), -7.5, dtype=dtype)
        box = view_box((n, n), layout, dtype)
        (pa, va), (pl, vl), (pr, vr) = place(a, layout), place(out0, layout), place(out0, layout)
        p0a, p0l, p0r = pa.clone(), pl.clone(), pr.clone()
        sp = torch.full((3 * n + 2,), -7.5, dtype=tdt, device="cuda")
        sip = torch.full((n + 4,), -7.5, dtype=tdt, device="cuda")
        s, si = sp[1:3 * n + 1:3], sip[2:n + 2]
        assert F.evd(va, s, si, vl, vr) == F.EVD_OK
        F.synchronize()
        guard_intact(pa, p0a, box, "evd A")
        assert np.array_equal(to_host(va), a), "A was written"
        guard_intact(pl, p0l, box, "evd UL")
        guard_intact(pr, p0r, box, "evd UR")
        sph, siph = sp.cpu().numpy(), sip.cpu().numpy()
        assert (np.delete(sph, np.arange(1, 3 * n + 1, 3)) == -7.5).all() and (siph[:2] == -7.5).all() and (siph[n + 2:] == -7.5).all()
        assert np.array_equal(s.cpu().numpy(), sd) and np.array_equal(si.cpu().numpy(), sid)
        assert np.array_equal(to_host(vl), uld) and np.array_equal(to_host(vr), urd)
        # row-major A
        _, sc, sic, ulc, urc = run(F, a, order="C")
        assert np.array_equal(sc, sd) and np.array_equal(sic, sid) and np.array_equal(ulc, uld) and np.array_equal(urc, urd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_blocking_caller_stream(dtype):
    """between a producer and a consumer on a non-blocking stream, with no host synchronisation of the test's own"""
    import torch

    F = init_gpu()
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for n in family_sizes(dtype):
        good, _ = make("normal01", n, dtype)
        stale, _ = make("normal01", n, dtype, seed=5)

        def fn(bufs):
            s = torch.full((n,), -7.5, dtype=tdt, device="cuda")
            si = torch.full((n,), -7.5, dtype=tdt, device="cuda")
            ul = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t()
            ur = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t()
            tag = F.evd(bufs["a"], s, si, ul, ur)
            return {"tag": tag, "s": s, "si": si, "ul": ul, "ur": ur}

        expected, got = ordered_call(fn, {"a": np.asfortranarray(good)}, {"a": np.asfortranarray(stale)})
        same_result(expected, got, f"evd on a non-blocking stream n={n}")
        assert expected["tag"] == F.EVD_OK


@pytest.mark.parametrize("dtype", DTYPES)
def test_eigenvalues_scale_with_powers_of_two(dtype):
    """the input times 2^k for the exponents of the EVD row of tests/range_cases.py: the eigenvalues are those of the unscaled input
    times 2^k, up to the residual bound (eigenvalues only: the back substitution squares entries of the Schur form)"""
    F = init_gpu()
    for n in family_sizes(dtype):
        a, _ = make("normal01", n, dtype)
        b = bound(a, ("normal01", n, np.dtype(dtype).name))
        na = np.linalg.norm(a.astype(np.float64))
        _, s0, si0, _, _ = run(F, a, left=False, right=False)
        lam0, _ = unpack(s0, si0, None)
        for k in RC.K["evd"][np.dtype(dtype)]:
            ak = RC.scaled(a, k)
            assert np.isfinite(ak).all() and (ak != 0).any()
            tag, s, si, _, _ = run(F, ak, left=False, right=False)
            assert tag == F.EVD_OK, (n, k)
            assert np.isfinite(s).all() and np.isfinite(si).all(), (n, k)
            lam, _ = unpack(s, si, None)
            back = np.ldexp(lam.real, -k) + 1j * np.ldexp(lam.imag, -k)
            assert match(back, lam0) <= b * na and match(lam0, back) <= b * na, (n, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_scratch_pool(dtype):
    """the arena on a pool filled with 0xFF, with 0x7F and without the fill: bit-identical outputs, and the fill has run"""
    F = init_gpu()
    try:
        for n in family_sizes(dtype):
            a, _ = make("normal01", n, dtype)
            b = bound(a, ("normal01", n, np.dtype(dtype).name))
            for host in (False, True):
                def call():
                    if not host:
                        return run(F, a)
                    s, si = np.full(n, -7.5, dtype=dtype), np.full(n, -7.5, dtype=dtype)
                    ul, ur = np.full((n, n), -7.5, dtype=dtype, order="F"), np.full((n, n), -7.5, dtype=dtype, order="F")
                    return F.evd(np.asfortranarray(a), s, si, ul, ur), s, si, ul, ur

                F.debug_scratch_fill(-1)
                base = call()
                F.debug_scratch_fill(0xFF)
                ff = call()
                F.synchronize()
                count, nbytes = F.debug_scratch_fill_stats()
                F.debug_scratch_fill(0x7F)
                sf = call()
                F.debug_scratch_fill(-1)
                # the arena alone holds H, Z, X and the working slices: more than three matrices were filled
                assert count > 0 and nbytes >= 3 * n * n * np.dtype(dtype).itemsize, (n, host, count, nbytes)
                for x, y, what in ((ff, sf, "0xFF against 0x7F"), (ff, base, "filled against unfilled")):
                    assert x[0] == y[0] == F.EVD_OK
                    for i in range(1, 5):
                        assert np.array_equal(x[i], y[i]), (n, host, what, ("s", "s_im", "ul", "ur")[i - 1])
                check_vectors(a, ff[1], ff[2], ff[3], ff[4], b, f"poisoned n={n} host={host}")
    finally:
        F.debug_scratch_fill(-1)
