"""General real EVD on the GPU (include/faer_hip.h section 2i, csrc/schur.hip): every size at which the Schur driver takes another
path (one leaf for n <= W, window sweeps above, W the window edge of the dtype), six kinds of input, the failure paths, and the
project's standing families (host operands, padded / offset / transposed views, a non-blocking caller stream, the ends of the
floating-point range, a poisoned scratch pool).

Bound.  For every input numpy's eig (LAPACK geev in the same dtype) is run on the CPU on the same matrix and two residuals of it
are measured: the Frobenius quotient r_np = |A V - V L|_F / (|A|_F |V|_F) and the worst column c_np = max_i |A v_i - l_i v_i|_2 /
(|A|_F |v_i|_2) (tests/evd_cases.py column_residuals, in fp64, every column scaled by its own largest entry).  The code is held to
4 max(r_np, n eps) and, per column and per vector set, to 4 max(c_np, n eps): the back substitution does not normalise, its columns
differ in norm by up to 1 / sqrt(min positive), and the quotient of Frobenius norms sees only the largest.  The factor 4 allows for a
different shift sequence and the missing early deflation, both backward stable at the same order.  Measured r_np (in units of
eps of the dtype) on the six normal or random kinds: float64, N(0,1): 0.5 (n = 2), 2.3 (3), 2.1 (95), 2.2 (96), 2.0 (97), 2.1 (195), 1.8
(337); symmetric 1.4 .. 1.8, triangular 0 .. 0.2, block diagonal 0 .. 1.8, cyclic 1.4 .. 2.9, normal 0.1 .. 1.8; c_np is at most 5.8
(normal, n = 96).  float32: at most 0.4 for every kind and size (numpy's eig of a float32 matrix rounds a double-precision result).
All are below n eps from n = 3 on, so the bounds in force are 4 n eps (n = 2: 8 eps, n = 1: 4 eps; the code's residuals there were 0.6
and 0).

The non-normal kinds (test_evd_non_normal_kinds), c_np / the code's worst column of either vector set / bound, in eps:
float64: graded_triangular and graded_quasi (n = 96) 0.00 / 0.00 / 384; jordan 0.16 / 7.3 / 120 (n = 30), 0.09 / 13.2 / 388 (97);
repeated_blocks 0.07 / 35.3 / 120 (30), 0.03 / 59.4 / 388 (97); rotated_* 0.97 .. 2.99 / 0.96 .. 3.13 / 4 n; scaled_similarity 0.00 /
0.21 .. 0.71 / 4 n.  float32 (c_np at most 0.04): graded_triangular 27.2 / 384, graded_quasi 14.8 / 384; jordan 7.3 / 120 (30), 15.2 /
516 (129); repeated_blocks 35.0 / 120 (30), 97.5 / 516 (129); rotated_* 0.39 .. 6.27 / 4 n; scaled_similarity 28.4 / 508 (127), 43.0
/ 516 (129), 52.2 / 1036 (259).  The largest component of the graded outputs is 1.2e152 (triangular) and 5.5e153 (quasi) under the
fp64 threshold 6.7e153, 3.9e18 under the fp32 threshold 9.2e18; unscaled, the vectors pass 1e290 (tests/test_evd_cases.py).

Spectrum.  Where the input is not defective the computed eigenvalues are assigned one to one to those of numpy's eig in fp64 of the
dtype-rounded input, each within radius_i = c n eps kappa_i |A|_F of its reference value (tests/evd_cases.py assign_spectrum,
reference_spectrum): kappa_i = |x_i| |y_i| / |y_i^H x_i| with the left vectors from inv(X), c = 4 for fp32 and 8 for fp64 inputs,
where the reference's own error is of the same order.  numpy's eig in the dtype of the input passes this on every such input
(tests/test_evd_cases.py).  A residual alone passes when an eigenpair is reported twice and another is missing."""
import ctypes as C

import numpy as np
import pytest

import evd_cases as ec
import range_cases as RC
from evd_cases import KINDS, make, unpack
from gpu_util import EPS, guard_intact, init_gpu, ordered_call, place, same_result, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
WEDGE = {np.dtype(np.float64): 96, np.dtype(np.float32): 128}


def sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [1, 2, 3, W - 1, W, W + 1, 2 * W + 3, {96: 337, 128: 449}[W]]


_PRINTED = set()


def bound(a, key):
    """4 max(Frobenius quotient of numpy's eig in the dtype of a, n eps), computed once per input"""
    return _bounds(a, key)[0]


def _bounds(a, key):
    bf, bc = ec.bounds(a, key)
    if key not in _PRINTED:
        _PRINTED.add(key)
        _, rf, rc = ec.numpy_same_dtype(a, key)
        e = float(EPS[a.dtype])
        print(f"numpy eig {key}: Frobenius quotient {rf / e:.2f} eps, worst column {rc / e:.2f} eps (n eps = {a.shape[0]} eps)")
    return bf, bc


def run(F, a, left=True, right=True, order="F", params=None):
    import torch

    n = a.shape[0]
    tdt = torch.float64 if a.dtype == np.float64 else torch.float32
    da = to_dev(a, order)
    s = torch.full((n,), -7.5, dtype=tdt, device="cuda")
    si = torch.full((n,), -7.5, dtype=tdt, device="cuda")
    ul = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if left else None
    ur = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if right else None
    tag = F.evd(da, s, si, ul, ur, params=params)
    F.synchronize()
    assert np.array_equal(to_host(da), a, equal_nan=True), "A was written"
    return tag, s.cpu().numpy(), si.cpu().numpy(), (ul.cpu().numpy() if left else None), (ur.cpu().numpy() if right else None)


def check_vectors(a, s, si, ul, ur, key, what):
    """both verdicts on every vector set given: the Frobenius quotient and the worst column, each against its bound of the case `key`"""
    bf, bc = _bounds(a, key)
    e = float(EPS[a.dtype])
    lam = None
    for side, u in (("right", ur), ("left", ul)):
        if u is None:
            continue
        assert np.isfinite(u).all(), (what, side)
        lam, V = unpack(s, si, u)
        assert (np.abs(V).max(axis=0) > 0).all(), (what, side, "a zero eigenvector column")
        cols = ec.column_residuals(a, lam, V, side)
        # (the Frobenius quotient squares the entries: columns scaled down together, by a power of two, keep it finite)
        r = ec.frobenius_quotient(a, lam, np.ldexp(V.real, -600) + 1j * np.ldexp(V.imag, -600), side) if np.abs(V).max() > 1e150 \
            else ec.frobenius_quotient(a, lam, V, side)
        print(f"{what} {side}: Frobenius quotient {r / e:.2f} eps (bound {bf / e:.0f} eps), worst column {cols.max() / e:.2f} eps at {cols.argmax()} "
              f"(bound {bc / e:.0f} eps)")
        assert r <= bf, (what, side, r, bf)
        assert cols.max() <= bc, (what, side, int(cols.argmax()), cols.max() / e, bc / e)
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
        key = (kind, n, np.dtype(dtype).name)
        b = bound(a, key)
        tag, s, si, ul, ur = run(F, a)
        assert tag == F.EVD_OK, what
        print(what, F.debug_evd_last_counts())
        lam = check_vectors(a, s, si, ul, ur, key, what)
        ref, radius = ec.reference_spectrum(a, key)
        assert ec.assign_spectrum(lam, ref, radius), (what, "the spectrum is not that of the fp64 reference")
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
            check_vectors(a, sl, sil, ull, None, key, what + " UL only")
            check_vectors(a, sr, sir, None, urr, key, what + " UR only")


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
    check_vectors(a, s, si, ul, ur, ("normal01", 40, np.dtype(dtype).name), "after a failure")


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
            check_vectors(a, s, si, ul, ur, ("normal01", n, np.dtype(dtype).name), f"host {layout} n={n}")


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
                check_vectors(a, ff[1], ff[2], ff[3], ff[4], ("normal01", n, np.dtype(dtype).name), f"poisoned n={n} host={host}")
    finally:
        F.debug_scratch_fill(-1)


def non_normal_sizes(kind, dtype):
    W = WEDGE[np.dtype(dtype)]
    if kind in ("graded_triangular", "graded_quasi"):
        return [ec.GUARD_N[np.dtype(dtype)]]
    if kind in ("jordan", "repeated_blocks"):
        return [30, W + 1]
    return [W - 1, W + 1, 2 * W + 3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ec.NEW_KINDS)
def test_evd_non_normal_kinds(kind, dtype):
    """the kinds of tests/evd_cases.py that reach the overflow guard and the divisor floor of the back substitution, and dense
    inputs with the same Schur forms: both vector sets under both verdicts, the spectrum of the non-defective ones assigned"""
    F = init_gpu()
    e = float(EPS[np.dtype(dtype)])
    for n in non_normal_sizes(kind, dtype):
        a, known, defective = ec.generate(kind, n, dtype)
        key = (kind, n, np.dtype(dtype).name)
        what = f"{kind} n={n} {np.dtype(dtype).name}"
        tag, s, si, ul, ur = run(F, a)
        assert tag == F.EVD_OK, what
        assert np.isfinite(s).all() and np.isfinite(si).all(), what
        print(what, F.debug_evd_last_counts())
        lam = check_vectors(a, s, si, ul, ur, key, what)  # (finite, no zero column, the pair layout of S_im, both verdicts)
        if not defective:
            ref, radius = ec.reference_spectrum(a, key)
            assert ec.assign_spectrum(lam, ref, radius), (what, "the spectrum is not that of the fp64 reference")
        if kind in ec.TRIANGULAR_KINDS:
            # a Schur form already: the real parts are the diagonal, an imaginary part is a product of two square roots
            assert np.array_equal(np.sort(s), np.sort(np.diag(a))), what
            assert ec.assign_spectrum(lam, known, 4 * e * np.abs(known).max()), what
        if kind in ("graded_triangular", "graded_quasi"):
            # the guard fired (tests/test_evd_cases.py: the unscaled vectors pass its threshold) and left no component beyond it
            big = ec.guard_threshold(dtype)
            for side, u in (("right", ur), ("left", ul)):
                print(f"{what} {side}: largest component {np.abs(u).max():.3e}, threshold {big:.3e}")
                assert np.abs(u).max() <= big * np.sqrt(n), (what, side)  # (U = Z X with Z orthogonal, here the identity)
            # each vector set alone: the left solve runs on the reversed transposed view, its guard sees other strides
            tagl, sl, sil, ull, _ = run(F, a, left=True, right=False)
            tagr, sr, sir, _, urr = run(F, a, left=False, right=True)
            assert tagl == F.EVD_OK and tagr == F.EVD_OK
            check_vectors(a, sl, sil, ull, None, key, what + " UL only")
            check_vectors(a, sr, sir, None, urr, key, what + " UR only")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ret", [0, 3, 64, 2 ** 63 + 5])
def test_shift_count_callback(ret, dtype):
    """a caller's recommended_shift_count that returns zero, an odd count, more than the window carries and a value that is
    negative as a long: the driver clamps each to an even count in [2, 2 max_bulges(W)] and the decomposition is as good"""
    F = init_gpu()
    W = WEDGE[np.dtype(dtype)]
    n = 2 * W + 3
    a, _ = make("normal01", n, dtype)
    key = ("normal01", n, np.dtype(dtype).name)
    calls = []

    def shift_count(dim, active):
        calls.append((dim, active))
        return ret

    cb = F.SHIFT_FN(shift_count)  # (alive until the call has returned)
    suf = "f64" if dtype == np.float64 else "f32"
    pf = getattr(F.lib(), f"libfaer_v0_23_EvdParams_{suf}")
    pf.restype = F.EvdParams
    params = pf()
    params.schur.recommended_shift_count = cb
    tag, s, si, ul, ur = run(F, a, params=params)
    assert tag == F.EVD_OK
    counts = F.debug_evd_last_counts()
    print(f"shift count {ret} n={n} {np.dtype(dtype).name}: {counts}, {len(calls)} calls, first {calls[:1]}")
    lam = check_vectors(a, s, si, ul, ur, key, f"shift count {ret} n={n}")
    ref, radius = ec.reference_spectrum(a, key)
    assert ec.assign_spectrum(lam, ref, radius)
    assert calls and all(d == n and W < m <= n for d, m in calls), calls[:4]
    assert counts["sweeps"] > 0 and len(calls) == counts["sweeps"]
    if ret == 64 and dtype == np.float32:
        # clamped to 2 max_bulges(W) = 42 shifts: the chain of 21 bulges fills the window exactly, s + 4 + 3 (nb - 1) = W, and the
        # first sweep, on an active block of m rows ((ihi - 2) - (ilo - 1) = m - 1), takes SweepPlan's number of window steps
        nb = 21
        assert (W - 3 * nb - 1) + 4 + 3 * (nb - 1) == W
        first = -(-((calls[0][1] - 1) + 3 * (nb - 1)) // (W - 3 * nb - 1))
        assert counts["window_steps"] >= first, (counts, first)
    del cb
