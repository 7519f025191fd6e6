"""generalized_evd on the GPU: every kind of tests/gevd_cases.py at n in {1, 2, 3, W - 1, W, W + 1, 2 W + 3, 3 W + 5} in both dtypes
under both verdicts (W = gevd_window_edge: up to W rows one LDS-resident leaf, beyond it multishift sweeps in windows), the `random`
kind as (A 2^ka, B 2^kb) at every row of gc.RANGE_SCALES, the kinds built for the eigenvector stage (gc.VECTOR_KINDS), and the standing
families: wanted / unwanted vector sets, host operands, padded / offset / row-major views, the poisoned scratch pool, a
non-blocking caller stream, non-finite inputs, custom shift counts, the counters."""
import ctypes as C

import numpy as np
import pytest

import gevd_cases as gc
from gpu_util import guard_intact, init_gpu, ordered_call, place, same_result, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu

DTYPES = gc.DTYPES
WEDGE = {np.dtype(np.float64): 64, np.dtype(np.float32): 96}
# state read-backs of one call beyond one per sweep and one per leaf: the finite check, the scan that finds nothing left, and the
# read of the kernels' counters at the end
READBACK_CONSTANT = 3


def sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [1, 2, 3, W - 1, W, W + 1, 2 * W + 3, 3 * W + 5]


def family_sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [3, W + 1]


def tdt_of(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def run(F, a, b, left=True, right=True, order="F", params=None):
    import torch

    n = a.shape[0]
    tdt = tdt_of(a.dtype)
    da, db = to_dev(a, order), to_dev(b, order)
    al, ai, be = (torch.full((n,), -7.5, dtype=tdt, device="cuda") for _ in range(3))
    ul = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if left else None
    ur = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() if right else None
    tag = F.generalized_evd(da, db, al, ai, be, ul, ur, params=params)
    F.synchronize()
    assert np.array_equal(to_host(da), a, equal_nan=True) and np.array_equal(to_host(db), b, equal_nan=True), "A or B was written"
    return tag, al.cpu().numpy(), ai.cpu().numpy(), be.cpu().numpy(), (ul.cpu().numpy() if left else None), (ur.cpu().numpy() if right else None)


CASES = [(kind, n, dtype) for dtype in DTYPES for kind in gc.KINDS for n in sizes(dtype) if gc.exists(kind, n)]


@pytest.mark.parametrize("kind,n,dtype", CASES, ids=[f"{k}-{n}-{np.dtype(d).name}" for k, n, d in CASES])
def test_kinds_pass_both_verdicts(kind, n, dtype):
    F = init_gpu()
    assert F.gevd_window_edge(dtype) == WEDGE[np.dtype(dtype)]
    a, b = gc.generate(kind, n, dtype)
    tag, al, ai, be, ul, ur = run(F, a, b)
    assert tag == F.GEVD_OK
    cnt = F.debug_gevd_last_counts()
    print(f"{kind} n={n} {np.dtype(dtype).name}: {cnt}")
    gc.check(kind, n, dtype, a, b, al, ai, be, ur, ul)
    assert (be >= 0).all()
    if kind == "triangular_pair":
        assert cnt["sweeps"] == 0
    if n <= WEDGE[np.dtype(dtype)]:
        assert cnt["window_steps"] == 0 and cnt["sweeps"] == 0
    elif kind != "triangular_pair" and n - (gc.singular_count(kind, n) if kind.startswith("singular_b") else 0) > WEDGE[np.dtype(dtype)]:  # a block of more than W rows takes multishift sweeps in windows
        assert cnt["sweeps"] > 0 and cnt["window_steps"] > cnt["sweeps"]
    if kind == "scaled":  # A 2^k, B 2^-k: every step scales by a power of two, so alpha and beta scale exactly
        _, al0, ai0, be0, _, _ = run(F, *gc.generate("random", n, dtype))
        assert np.array_equal(np.ldexp(al0, gc.SCALE_K), al) and np.array_equal(np.ldexp(ai0, gc.SCALE_K), ai)
        assert np.array_equal(np.ldexp(be0, -gc.SCALE_K), be)
    if kind.startswith("singular_b"):
        assert cnt["infinite_deflations"] >= gc.singular_count(kind, n)
    assert cnt["readbacks"] <= cnt["sweeps"] + cnt["leaves"] + READBACK_CONSTANT
    if kind == "identity_b":
        lam = (al.astype(np.float64) + 1j * ai) / be
        ref = np.linalg.eigvals(a.astype(np.float64))
        d = np.abs(lam[:, None] - ref[None, :]).min(axis=1).max()
        assert d <= 1e3 * n * gc.eps_of(dtype) * np.linalg.norm(a.astype(np.float64))


def range_sizes(dtype):
    W = WEDGE[np.dtype(dtype)]
    return [W - 1, W + 1, 2 * W + 3]


_UNSCALED = {}


def unscaled_run(F, n, dtype, vectors=True):
    """the result on the `random` pair itself, once per size and dtype"""
    key = (n, np.dtype(dtype).name, vectors)
    if key not in _UNSCALED:
        a, b = gc.generate("random", n, dtype)
        _UNSCALED[key] = run(F, a, b, vectors, vectors) + (F.debug_gevd_last_counts(),)
    return _UNSCALED[key]


def qr_fast_path(b):
    nz = np.abs(b[b != 0]).astype(np.float64)
    return bool(((nz >= 1e-120) & (nz <= 1e120)).all())


def range_row(F, n, dtype, ka, kb, vectors):
    """(A 2^ka, B 2^kb): GEVD_OK, the counters, both verdicts on unscaled quantities, and the unscaled call's alpha 2^ka,
    beta 2^kb and vectors bit for bit"""
    W = WEDGE[np.dtype(dtype)]
    _, _, a, b = gc.range_generate(n, dtype, ka, kb)
    tag, al, ai, be, ul, ur = run(F, a, b, vectors, vectors)
    cnt = F.debug_gevd_last_counts()
    print(f"random n={n} {np.dtype(dtype).name} 2^({ka}, {kb}): tag {tag}, {cnt}")
    assert tag == F.GEVD_OK
    gc.range_check(n, dtype, ka, kb, al, ai, be, ur, ul)
    assert (be >= 0).all()
    if n <= W:
        assert cnt["window_steps"] == 0 and cnt["sweeps"] == 0
    else:
        assert cnt["sweeps"] > 0 and cnt["window_steps"] > cnt["sweeps"]
    assert cnt["readbacks"] <= cnt["sweeps"] + cnt["leaves"] + READBACK_CONSTANT
    tag0, al0, ai0, be0, ul0, ur0, cnt0 = unscaled_run(F, n, dtype, vectors)
    assert tag0 == F.GEVD_OK and cnt == cnt0
    exact = [np.array_equal(np.ldexp(al0, ka), al), np.array_equal(np.ldexp(ai0, ka), ai), np.array_equal(np.ldexp(be0, kb), be)]
    if vectors:
        exact += [np.array_equal(ul0, ul), np.array_equal(ur0, ur)]
    print(f"random n={n} {np.dtype(dtype).name} 2^({ka}, {kb}): bit-exact alpha, alpha_im, beta, UL, UR: {exact}")
    # Stages 1 to 3 scale exactly at every row (tests/test_qz_host.py).  Stage 0, the QR of B, has two paths in fp64: a nonzero
    # entry of B outside [1e-120, 1e120] takes the general one (copy_guard_kernel of csrc/qr.hip), whose norms round differently,
    # so there the whole call is compared bit for bit only with a B on the same path
    if np.dtype(dtype) == np.float32 or qr_fast_path(b):
        assert all(exact)


RANGE = [(n, dtype, group, ka, kb) for dtype in DTYPES for n in range_sizes(dtype) for group, ka, kb in gc.range_rows(dtype)]


@pytest.mark.parametrize("n,dtype,group,ka,kb", RANGE, ids=[f"{n}-{np.dtype(d).name}-{g}-{ka}-{kb}" for n, d, g, ka, kb in RANGE])
def test_range_rows(n, dtype, group, ka, kb):
    """every row of gc.RANGE_SCALES at n = W - 1 (one leaf), W + 1 and 2 W + 3 (windows)"""
    assert gc.range_representable(n, dtype, ka, kb)
    range_row(init_gpu(), n, dtype, ka, kb, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_range_row_eigenvalues_only(dtype):
    """the widest row apart, neither vector set wanted: lambda itself is not representable, (alpha, beta) is"""
    ka, kb = gc.RANGE_SCALES[np.dtype(dtype)]["beyond"][2]
    range_row(init_gpu(), WEDGE[np.dtype(dtype)] + 1, dtype, ka, kb, False)


VECTOR = [(kind, gc.GUARD_N if kind in gc.TRIANGLE_KINDS else WEDGE[np.dtype(dtype)] + 1, dtype) for dtype in DTYPES for kind in gc.VECTOR_KINDS]


@pytest.mark.parametrize("kind,n,dtype", VECTOR, ids=[f"{k}-{n}-{np.dtype(d).name}" for k, n, d in VECTOR])
def test_vector_kinds(kind, n, dtype):
    """the kinds built for gevd_vec_kernel: the overflow rescale (graded_triangular_pair at the size where it fires), the pivot floor
    at every divisor (jordan_pair), the vectors of infinite eigenvalues (infinite_in_triangle), and their rotations at W + 1;
    triangular pairs take zero sweeps and keep their diagonals (gc.check asserts alpha and beta exactly)"""
    F = init_gpu()
    a, b = gc.generate(kind, n, dtype)
    tag, al, ai, be, ul, ur = run(F, a, b)
    cnt = F.debug_gevd_last_counts()
    print(f"{kind} n={n} {np.dtype(dtype).name}: tag {tag}, {cnt}")
    assert tag == F.GEVD_OK
    for x in (al, ai, be, ul, ur):
        assert np.isfinite(x).all()
    # (the QR of a singular triangular B is another triangle: the diagonals of infinite_in_triangle are asserted on the host alone)
    gc.check(kind, n, dtype, a, b, al, ai, be, ur, ul, stage0_identity=kind != "infinite_in_triangle")
    assert (be >= 0).all()
    if kind == "infinite_in_triangle":
        assert cnt["infinite_deflations"] >= len(gc.infinite_rows(n))
    if kind in gc.TRIANGLE_KINDS:
        assert cnt["sweeps"] == 0 and cnt["window_steps"] == 0
    elif kind != "rotated_infinite_in_triangle":  # (three infinite eigenvalues deflate first: the block left may fit one leaf)
        assert cnt["sweeps"] > 0 and cnt["window_steps"] > cnt["sweeps"]
    assert cnt["readbacks"] <= cnt["sweeps"] + cnt["leaves"] + READBACK_CONSTANT


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_vector_sets(dtype):
    """all four combinations of wanted and unwanted UL, UR; with neither wanted the eigenvalues are those of the full call to the radius"""
    F = init_gpu()
    for n in family_sizes(dtype):
        a, b = gc.generate("random", n, dtype)
        ref = gc.reference("random", n, dtype)
        for left, right in ((True, True), (True, False), (False, True), (False, False)):
            tag, al, ai, be, ul, ur = run(F, a, b, left, right)
            assert tag == F.GEVD_OK
            gc.check("random", n, dtype, a, b, al, ai, be, ur, ul, verbose=False)
            alc, _ = gc.unpack(al, ai, be, None)
            assert gc.assign_pairs(alc, be.astype(np.float64), ref)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_host_operands(dtype):
    F = init_gpu()
    for n in family_sizes(dtype):
        a, b = gc.generate("random", n, dtype)
        _, ald, aid, bed, uld, urd = run(F, a, b)
        for order in ("F", "C"):
            ha, hb = np.array(a, order=order), np.array(b, order=order)
            al, ai, be = (np.full(n, -7.5, dtype=dtype) for _ in range(3))
            ul, ur = np.full((n, n), -7.5, dtype=dtype, order="F"), np.full((n, n), -7.5, dtype=dtype, order="C")
            assert F.generalized_evd(ha, hb, al, ai, be, ul, ur) == F.GEVD_OK
            assert np.array_equal(ha, a) and np.array_equal(hb, b)
            for x, y in ((al, ald), (ai, aid), (be, bed), (ul, uld), (ur, urd)):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", ["sub", "rowpad", "mat"])
def test_device_views(layout, dtype):
    """padded and offset device views of every operand and row-major A, B: guard cells intact, A and B bit-identical, values those of
    plain operands"""
    import torch

    F = init_gpu()
    tdt = tdt_of(dtype)
    for n in family_sizes(dtype):
        a, b = gc.generate("random", n, dtype)
        _, ald, aid, bed, uld, urd = run(F, a, b)
        out0 = np.full((n, n), -7.5, dtype=dtype)
        box = view_box((n, n), layout, dtype)
        (pa, va), (pb, vb), (pl, vl), (pr, vr) = place(a, layout), place(b, layout), place(out0, layout), place(out0, layout)
        snaps = [p.clone() for p in (pa, pb, pl, pr)]
        sp = torch.full((3 * n + 2,), -7.5, dtype=tdt, device="cuda")
        al, ai, be = sp[1:3 * n + 1:3], torch.full((n,), -7.5, dtype=tdt, device="cuda"), torch.full((n,), -7.5, dtype=tdt, device="cuda")
        assert F.generalized_evd(va, vb, al, ai, be, vl, vr) == F.GEVD_OK
        F.synchronize()
        for p, p0, what in zip((pa, pb, pl, pr), snaps, ("A", "B", "UL", "UR")):
            guard_intact(p, p0, box, f"generalized_evd {what}")
        assert np.array_equal(to_host(va), a) and np.array_equal(to_host(vb), b), "A or B was written"
        assert (np.delete(sp.cpu().numpy(), np.arange(1, 3 * n + 1, 3)) == -7.5).all()
        assert np.array_equal(al.cpu().numpy(), ald) and np.array_equal(ai.cpu().numpy(), aid) and np.array_equal(be.cpu().numpy(), bed)
        assert np.array_equal(to_host(vl), uld) and np.array_equal(to_host(vr), urd)
        _, alc, aic, bec, ulc, urc = run(F, a, b, order="C")
        assert np.array_equal(alc, ald) and np.array_equal(bec, bed) and np.array_equal(ulc, uld) and np.array_equal(urc, urd)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_poisoned_scratch_pool(dtype):
    """the arena on a pool filled with 0xFF and with 0x7F: the verdicts pass, no NaN appears, the outputs are bit-identical"""
    F = init_gpu()
    try:
        for n in family_sizes(dtype):
            a, b = gc.generate("random", n, dtype)
            for host in (False, True):
                def call():
                    if not host:
                        return run(F, a, b)
                    al, ai, be = (np.full(n, -7.5, dtype=dtype) for _ in range(3))
                    ul, ur = np.full((n, n), -7.5, dtype=dtype, order="F"), np.full((n, n), -7.5, dtype=dtype, order="F")
                    return F.generalized_evd(np.asfortranarray(a), np.asfortranarray(b), al, ai, be, ul, ur), al, ai, be, ul, ur

                F.debug_scratch_fill(0xFF)
                ff = call()
                F.synchronize()
                count, nbytes = F.debug_scratch_fill_stats()
                F.debug_scratch_fill(0x7F)
                sf = call()
                F.debug_scratch_fill(-1)
                assert count > 0 and nbytes >= 5 * n * n * np.dtype(dtype).itemsize, (n, host, count, nbytes)
                assert ff[0] == sf[0] == F.GEVD_OK
                for i in range(1, 6):
                    assert np.isfinite(ff[i]).all() and np.array_equal(ff[i], sf[i]), (n, host, i)
                gc.check("random", n, dtype, a, b, ff[1], ff[2], ff[3], ff[5], ff[4], verbose=False)
    finally:
        F.debug_scratch_fill(-1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_non_blocking_caller_stream(dtype):
    """between a producer and a consumer on a non-blocking stream, with no host synchronisation of the test's own"""
    import torch

    F = init_gpu()
    tdt = tdt_of(dtype)
    for n in family_sizes(dtype):
        (ga, gb), (sa, sb) = gc.generate("random", n, dtype), gc.generate("random", n, dtype, seed=5)

        def fn(bufs):
            al, ai, be = (torch.full((n,), -7.5, dtype=tdt, device="cuda") for _ in range(3))
            ul = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t()
            ur = torch.full((n, n), -7.5, dtype=tdt, device="cuda").t()
            tag = F.generalized_evd(bufs["a"], bufs["b"], al, ai, be, ul, ur)
            return {"tag": tag, "alpha": al, "alpha_im": ai, "beta": be, "ul": ul, "ur": ur}

        expected, got = ordered_call(fn, {"a": np.asfortranarray(ga), "b": np.asfortranarray(gb)}, {"a": np.asfortranarray(sa), "b": np.asfortranarray(sb)})
        same_result(expected, got, f"generalized_evd on a non-blocking stream n={n}")
        assert expected["tag"] == F.GEVD_OK
        gc.check("random", n, dtype, ga, gb, got["alpha"], got["alpha_im"], got["beta"], got["ur"], got["ul"], verbose=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_non_finite_input(dtype):
    F = init_gpu()
    n = 17
    a, b = gc.generate("random", n, dtype)
    for which, bad in (("a", np.nan), ("b", np.inf)):
        a2, b2 = a.copy(), b.copy()
        (a2 if which == "a" else b2)[3, 5] = bad
        tag, al, ai, be, ul, ur = run(F, a2, b2)
        assert tag == F.GEVD_NO_CONVERGENCE
        for x in (al, ai, be, ul, ur):
            assert np.isnan(x).all()
        tag, al, ai, be, ul, ur = run(F, a, b)
        assert tag == F.GEVD_OK
        gc.check("random", n, dtype, a, b, al, ai, be, ur, ul, verbose=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_custom_shift_counts(dtype):
    """a shift-count callback returning 0, 3, 64 and 2^63 + 5: the call still passes (the count is clamped where it is used)"""
    F = init_gpu()
    n = WEDGE[np.dtype(dtype)] + 1
    a, b = gc.generate("random", n, dtype)
    pf = getattr(F.lib(), f"libfaer_v0_23_GevdParams_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")
    pf.restype = F.GevdParams
    steps = {}
    for count in (0, 3, 64, 2 ** 63 + 5):
        calls = []

        def fn(n_, m_, c=count, calls=calls):
            calls.append((n_, m_))
            return c

        cb = F.SHIFT_FN(fn)
        p = pf()
        p.schur.recommended_shift_count = cb
        tag, al, ai, be, ul, ur = run(F, a, b, params=p)
        assert tag == F.GEVD_OK
        cnt = F.debug_gevd_last_counts()
        assert calls and all(c[0] == n for c in calls) and len(calls) == cnt["sweeps"] and cnt["window_steps"] > 0
        steps[count] = (cnt["sweeps"], cnt["window_steps"])
        gc.check("random", n, dtype, a, b, al, ai, be, ur, ul, verbose=False)
    assert steps[0] == steps[3]  # both clamp to one bulge
    assert steps[64] == steps[2 ** 63 + 5] != steps[0]  # both clamp to the most bulges a window carries
