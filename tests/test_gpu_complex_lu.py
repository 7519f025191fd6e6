"""The complex partial-pivot LU on the GPU (cgetrf.hip): factor, solve, transpose solve for c32 / c64.

Yardsticks: tests/complex_lu_ref.py (test_complex_lu_abi.py shows on the CPU that the numpy restatement stays inside them on the
shapes used here).  Shapes are placed around W and the leaf limit read from debug_clu_shape; debug_clu_last says which path ran.

Bit-for-bit comparisons between memory layouts: the panel kernels and the interchanges do the same arithmetic in every layout.  The
complex GEMM runs a destination with unit column stride as its transpose (cgemm.hip), which adds the two halves of an imaginary part
in the other order, so a row-major matrix is compared bit for bit where no GEMM runs (one panel), and by pivots, backward error and
the factor bound of test 1 where one does."""
import functools

import numpy as np
import pytest

import complex_lu_ref as ref
from gpu_util import fa, guard_intact, init_gpu, ordered_call, same_result, to_dev, to_host, view_box

pytestmark = pytest.mark.gpu

CDTYPES = [np.complex64, np.complex128]
SHAPES = [(1, 1), (2, 2), (3, 3), (31, 31), (33, 33), ("W", "W"), ("W+1", "W+1"), (129, 129), (257, 257), (300, 8), (8, 300), (40, 17), (17, 40),
          ("leaf", "W"), ("leaf+1", "W"), (2000, 64), (5000, 40), (700, 700)]


def resolve(shape, dtype):
    w, leaf = fa().debug_clu_shape(dtype)
    names = {"W": w, "W+1": w + 1, "leaf": leaf, "leaf+1": leaf + 1}
    return tuple(names.get(s, s) for s in shape)


@functools.lru_cache(maxsize=None)
def reference(m, n, dtype):
    """(A, packed LU, perm, count) of the restatement; computed once per shape and type, never modified"""
    a = ref.gaussian(m, n, dtype, 7 + m + 3 * n)
    lu, perm, count = ref.lu_unblocked(a)
    return a, lu, perm, count


def factor(F, a, index_dtype=np.uint64):
    d = to_dev(a)
    perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(d, index_dtype)
    return np.array(to_host(d)), perm.astype(np.int64), perm_inv.astype(np.int64), int(nt)


def check_factor(a, lu, perm, perm_inv, nt, want=None, what=""):
    m, n = a.shape
    k = min(m, n)
    eps = np.finfo(a.dtype).eps
    assert np.array_equal(perm_inv[perm], np.arange(m)), what
    rec, moved = ref.records_from_perm(perm, k)
    assert moved == nt, (what, moved, nt)
    e = ref.lu_backward_error(a, lu, perm)
    print(f"{what}: backward error {e:.2e} of the bound")
    assert e <= 1.0, (what, e)
    low = np.abs(np.tril(lu[:, :k], -1)).max(initial=0.0)
    assert low <= np.sqrt(2) * (1 + 4 * eps), (what, low)
    if want is not None:
        wlu, wperm = want
        assert np.array_equal(perm, wperm), what
        kappa = np.linalg.cond(a[perm][:k, :k].astype(np.complex128))
        tol = 12 * max(m, n) * eps * kappa * max(1.0, np.abs(wlu).max())
        d = np.abs(lu.astype(np.complex128) - wlu.astype(np.complex128)).max()
        assert d <= tol, (what, d, tol)


# ---- 1. factor against the reference
@pytest.mark.parametrize("index_dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_factor_vs_reference(shape, dtype, index_dtype):
    F = init_gpu()
    m, n = resolve(shape, dtype)
    a, wlu, wperm, _ = reference(m, n, dtype)
    lu, perm, perm_inv, nt = factor(F, a, index_dtype)
    strict = dtype == np.complex128 or m <= 300  # a larger c32 case may resolve a near tie differently: judged by the two bounds alone
    check_factor(a, lu, perm, perm_inv, nt, (wlu, wperm) if strict else None, f"{m}x{n} {np.dtype(dtype).name}")


# ---- 2. path taken
def expected_last(m, n, w, leaf):
    """the driver's panels are the blocks of W columns; a panel of more than `leaf` rows takes one launch per column and a prologue;
    a panel's interchanges are one launch when there are other columns and at least two rows"""
    k = min(m, n)
    panels = [(m - c0, min(w, k - c0)) for c0 in range(0, k, w)]
    step = [p for p in panels if p[0] > leaf]
    return {"leaf_panels": len(panels) - len(step), "step_panels": len(step), "step_launches": sum(pw + 1 for _, pw in step),
            "swap_launches": sum(1 for mp, pw in panels if n > pw and mp >= 2)}


@pytest.mark.parametrize("dtype", CDTYPES)
def test_path_taken(dtype):
    F = init_gpu()
    w, leaf = F.debug_clu_shape(dtype)
    for m, n in ((leaf, w), (leaf + 1, w), (5000, 40), (700, 700), (8, 300)):
        factor(F, reference(m, n, dtype)[0])
        last = F.debug_clu_last()
        assert last == expected_last(m, n, w, leaf), (m, n, last)
        if (m, n) == (leaf, w):
            assert last == {"leaf_panels": 1, "step_panels": 0, "step_launches": 0, "swap_launches": 0}
        if (m, n) == (5000, 40):
            assert last["leaf_panels"] == 0 and last["step_panels"] >= 1 and last["step_launches"] == 40 + last["step_panels"]
        if (m, n) == (700, 700):
            assert last["leaf_panels"] >= 1 and last["step_panels"] >= 1


# ---- 3. pivot rule
@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("m", [40, 5000])
def test_abs1_not_modulus(m, dtype):
    F = init_gpu()
    a = np.array(reference(m, 8, dtype)[0]) * dtype(0.125)
    a[3, 0] = 5  # abs1 5, modulus 5
    a[m - 7, 0] = 3 + 3j  # abs1 6, modulus 4.24
    lu, perm, perm_inv, nt = factor(F, a)
    assert perm[0] == m - 7
    wlu, wperm, _ = ref.lu_unblocked(a)
    check_factor(a, lu, perm, perm_inv, nt, (wlu, wperm), f"abs1 {m}")


@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("m,rows", [(250, (5, 40)), (250, (20, 200)), (5000, (20, 4000)), (5000, (300, 301))])
def test_ties_go_to_the_smaller_row(m, rows, dtype):
    """equal abs1 in one wave (rows 5 and 40 of a leaf), in different waves of one workgroup (20 and 200), in different workgroups of
    a column-step panel (20 and 4000), and next to each other; in column 0 and -- after an exact first step -- in column 1"""
    F = init_gpu()
    for col in (0, 1):
        a = np.array(reference(m, 8, dtype)[0]) * dtype(0.0625)
        if col == 1:  # column 0 = 8 e_0: step 0 keeps row 0 and leaves the other rows untouched
            a[:, 0] = 0
            a[0, :] = 0
            a[0, 0] = 8
        lo, hi = rows
        a[lo, col] = 2 - 2j
        a[hi, col] = 4  # the same abs1, another modulus
        lu, perm, perm_inv, nt = factor(F, a)
        assert perm[col] == lo, (col, perm[col])
        a[lo, col], a[hi, col] = 4j, 1 + 3j
        lu, perm, perm_inv, nt = factor(F, a)
        assert perm[col] == lo, (col, perm[col])
        wlu, wperm, _ = ref.lu_unblocked(a)
        check_factor(a, lu, perm, perm_inv, nt, (wlu, wperm), f"ties {m} {rows} column {col}")


@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("m", [40, 300, 5000])
def test_zero_column_and_nan(m, dtype):
    F = init_gpu()
    a = np.array(reference(m, 8, dtype)[0])
    a[:, 0] = 0
    lu, perm, _, _ = factor(F, a)
    wlu, wperm, _ = ref.lu_unblocked(a)
    assert perm[0] == 0 and np.array_equal(perm, wperm)
    assert np.array_equal(np.isfinite(lu), np.isfinite(wlu))
    assert not np.isfinite(lu[1:, 0]).any()
    b = np.array(reference(m, 8, dtype)[0])
    b[m - 2, 0] = np.nan  # below the diagonal: never the pivot of column 0, and its row is never chosen later
    lu, perm, _, _ = factor(F, b)
    wlu, wperm, _ = ref.lu_unblocked(b)
    assert perm[0] != m - 2 and m - 2 not in perm[:8].tolist()
    assert np.array_equal(perm, wperm)
    assert np.array_equal(np.isfinite(lu), np.isfinite(wlu))


# ---- 4. exact case
@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("n", [40, 130])
def test_exact_case(n, dtype):
    F = init_gpu()
    a, l, u = ref.exact_case(n, dtype)
    lu, perm, perm_inv, nt = factor(F, a)
    assert nt == 0 and np.array_equal(perm, np.arange(n)) and np.array_equal(perm_inv, np.arange(n))
    gl, gu = ref.split(lu)
    assert np.array_equal(gl, l) and np.array_equal(gu, u)


# ---- 5. solves
def op_of(a, transpose, conj):
    x = a.conj() if conj else a
    return x.T if transpose else x


@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("nrhs", [1, 33])
@pytest.mark.parametrize("n", [1, 33, 64, 65, 300])
def test_solves(n, nrhs, dtype):
    F = init_gpu()
    a = reference(n, n, dtype)[0]
    b = ref.gaussian(n, nrhs, dtype, 90 + n + nrhs)
    d = to_dev(a)
    perm, perm_inv, _ = F.partial_piv_lu_factor_in_place(d)
    lu = np.array(to_host(d))
    g = ref.abs_lu(lu, perm)  # |L||U| in the row order of A
    sols = []
    for transpose in (False, True):
        for conj in (False, True):
            x = to_dev(b)
            F.partial_piv_lu_solve_in_place(d, perm, perm_inv, x, transpose=transpose, conj=conj)
            xs = np.array(to_host(x))
            e = ref.solve_error(op_of(a, transpose, conj), g.T if transpose else g, xs, b, dtype)
            print(f"n={n} nrhs={nrhs} transpose={transpose} conj={conj}: {e:.2e} of the bound")
            assert e <= 1.0, (transpose, conj, e)
            sols.append(xs)
    if n > 1:  # (a 1 x 1 transpose is itself)
        for i in range(4):
            for k in range(i + 1, 4):
                assert not np.array_equal(sols[i], sols[k]), (i, k)
    else:
        assert not np.array_equal(sols[0], sols[1])


# ---- 6. views and operands
def place_c(a, layout):
    """(parent, view, box, parent snapshot on the host) on the device: the complex matrix `a` inside a guarded parent (gpu_util.view_box)"""
    import torch

    box = view_box(a.shape, layout, a.dtype)
    rdt = np.float64 if a.dtype == np.complex128 else np.float32
    guard = np.array([0x7FF8DEADBEEF0BAD], np.int64).view(np.float64)[0] if rdt == np.float64 else np.array([0x7FC0BEEF], np.int32).view(np.float32)[0]
    flat = np.empty(box.base + box.numel, dtype=a.dtype)
    flat.view(rdt)[:] = guard
    parent = np.lib.stride_tricks.as_strided(flat[box.base:], box.shape, tuple(s * a.itemsize for s in box.pstrides))
    parent[box.rows(), box.cols()] = a
    dev = torch.from_numpy(flat).cuda()
    dparent = dev.as_strided(box.shape, box.pstrides, box.base)
    return dparent, dparent[box.rows(), box.cols()], box, np.array(parent)


def guards_ok(dparent, parent0, box, what):
    fa().synchronize()
    now = dparent.cpu().numpy()
    guard_intact(np.ascontiguousarray(now.real), np.ascontiguousarray(parent0.real), box, what + " (re)")
    guard_intact(np.ascontiguousarray(now.imag), np.ascontiguousarray(parent0.imag), box, what + " (im)")


def raw_bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64 if x.dtype == np.complex128 else np.int32)


@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("m,n", [(300, 20), (700, 24), (150, 150)])
def test_views_and_operands(m, n, dtype):
    """one panel on the leaf (300 x 20 in c32) and on the column-step kernels (700 x 24; 300 x 20 in c64); 150 x 150: five panels with
    solves and products"""
    F = init_gpu()
    a = reference(m, n, dtype)[0]
    lu0, perm0, perm_inv0, nt0 = factor(F, a)
    multi = n > F.debug_clu_shape(dtype)[0]

    def same(lu, perm, nt, what):
        assert np.array_equal(perm, perm0) and nt == nt0, what
        assert np.array_equal(raw_bits(lu), raw_bits(lu0)), what

    for layout in ("sub", "mat", "odd", "rowpad", "step2"):
        dparent, view, box, parent0 = place_c(np.array(a), layout)
        perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(view)
        guards_ok(dparent, parent0, box, f"factor {m}x{n}")
        lu = np.array(to_host(view))
        if layout == "rowpad" and multi:  # the products run transposed: see the module docstring
            check_factor(a, lu, perm.astype(np.int64), perm_inv.astype(np.int64), int(nt), (lu0, perm0), f"rowpad {m}x{n}")
        else:
            same(lu, perm.astype(np.int64), int(nt), layout)
    # reversed rows on the device: the view of a flipped matrix, handed over with a negative row stride
    d = to_dev(np.array(a)[::-1])
    suf, _, isz = F._dtype_suffix(d)
    fwd, bwd = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    L = F.lib()
    st = getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_u64_{suf}")(
        F.MatMut(d.data_ptr() + (m - 1) * d.stride(0) * isz, m, n, -d.stride(0), d.stride(1)), F.SliceMut(fwd.ctypes.data, m), F.SliceMut(bwd.ctypes.data, m),
        F.PAR_SEQ, F.MemAlloc(None, 0), getattr(L, f"libfaer_v0_23_PartialPivLuParams_{suf}")())
    assert st.tag == 0
    same(np.array(to_host(d))[::-1], fwd.astype(np.int64), int(st.transposition_count), "reversed rows")
    # host operands: column major, and a reversed-row view of a flipped host matrix (packed through the staging path)
    h = np.array(a, order="F")
    perm, _, nt = F.partial_piv_lu_factor_in_place(h)
    same(h, perm.astype(np.int64), int(nt), "host")
    hr = np.array(np.array(a)[::-1], order="F")
    perm, _, nt = F.partial_piv_lu_factor_in_place(hr[::-1])
    same(hr[::-1], perm.astype(np.int64), int(nt), "host reversed")
    if m != n:
        return
    # solves: lu in every layout, rhs as a padded and offset view and as a host operand
    b = ref.gaussian(n, 5, dtype, 11)
    dl = to_dev(lu0)
    x0 = {}
    for transpose in (False, True):
        x = to_dev(b)
        F.partial_piv_lu_solve_in_place(dl, perm0.astype(np.uint64), perm_inv0.astype(np.uint64), x, transpose=transpose, conj=True)
        x0[transpose] = np.array(to_host(x))
    for layout in ("sub", "rowpad", "step2"):
        lparent, lview, lbox, lparent0 = place_c(lu0, layout)
        for transpose in (False, True):
            xparent, xview, xbox, xparent0 = place_c(b, "sub")
            F.partial_piv_lu_solve_in_place(lview, perm0.astype(np.uint64), perm_inv0.astype(np.uint64), xview, transpose=transpose, conj=True)
            guards_ok(xparent, xparent0, xbox, "solve rhs")
            guards_ok(lparent, lparent0, lbox, "solve lu")
            assert np.array_equal(raw_bits(np.array(to_host(xview))), raw_bits(x0[transpose])), (layout, transpose)
    for transpose in (False, True):
        xh = np.array(b, order="F")
        F.partial_piv_lu_solve_in_place(np.array(lu0, order="F"), perm0.astype(np.uint64), perm_inv0.astype(np.uint64), xh, transpose=transpose, conj=True)
        assert np.array_equal(raw_bits(xh), raw_bits(x0[transpose])), ("host", transpose)


# ---- 7. stream
@pytest.mark.parametrize("dtype", CDTYPES)
def test_factor_and_solve_on_a_caller_stream(dtype):
    F = init_gpu()
    n = 700
    good = {"a": np.array(reference(n, n, dtype)[0]), "b": ref.gaussian(n, 3, dtype, 1001)}
    stale = {"a": ref.gaussian(n, n, dtype, 2000), "b": ref.gaussian(n, 3, dtype, 2001)}

    def fn(bufs):
        perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(bufs["a"])
        F.partial_piv_lu_solve_in_place(bufs["a"], perm, perm_inv, bufs["b"], transpose=True, conj=True)
        return {"lu": bufs["a"], "x": bufs["b"], "perm": perm, "perm_inv": perm_inv, "nt": nt}

    expected, got = ordered_call(fn, good, stale)
    assert sorted(expected["perm"].tolist()) == list(range(n))
    same_result(expected, got, f"complex lu {n}")
    assert np.array_equal(raw_bits(expected["lu"]), raw_bits(got["lu"])) and np.array_equal(raw_bits(expected["x"]), raw_bits(got["x"]))


# ---- 8. poisoned pool
@pytest.mark.parametrize("dtype", CDTYPES)
def test_poisoned_pool(dtype):
    F = init_gpu()
    cases = [reference(700, 700, dtype)[0], reference(5000, 40, dtype)[0]]
    b = ref.gaussian(700, 3, dtype, 12)

    def run():
        out = []
        for a in cases:
            d = to_dev(a)
            perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(d)
            out += [raw_bits(np.array(to_host(d))), perm, int(nt)]
            if a.shape[0] == a.shape[1]:
                x = to_dev(b)
                F.partial_piv_lu_solve_in_place(d, perm, perm_inv, x)
                out.append(raw_bits(np.array(to_host(x))))
        return out

    base = run()
    try:
        for fill in (0xFF, 0x7F):
            F.debug_scratch_fill(fill)
            got = run()
            assert F.debug_scratch_fill_stats()[0] > 0
            for e, g in zip(base, got):
                assert np.array_equal(e, g), fill
    finally:
        F.debug_scratch_fill(-1)


# ---- 9. the real family is untouched
def test_real_lu_is_unchanged_by_a_complex_call():
    F = init_gpu()
    a = np.asfortranarray(np.random.default_rng(257).standard_normal((257, 257)))

    def real():
        d = to_dev(a)
        perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(d)
        return np.array(to_host(d)).view(np.int64), perm, perm_inv, int(nt)

    before = real()
    factor(F, reference(700, 700, np.complex128)[0])
    factor(F, reference(300, 8, np.complex64)[0])
    after = real()
    for e, g in zip(before, after):
        assert np.array_equal(e, g)
