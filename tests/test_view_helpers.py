"""CPU tests of the view infrastructure of tests/test_gpu_views.py (tests/gpu_util.py: place_host / place, guard_intact):
the layouts have the strides and offsets they claim, the oracle computes the same bits on a padded or offset view as on
a dense array of the same major order and writes nothing outside it -- which is what entitles the GPU tests to judge a
device view by the oracle's run on place_host of the same layout -- and guard_intact reports every kind of stray write."""
import numpy as np
import pytest

from gpu_util import GUARD_BITS, LAYOUTS, bits, guard_fill, guard_intact, place_host, view_box
from oracle import oracle as O

DTYPES = [np.float64, np.float32]


# ------------------------------------------------------------------------------------------------ place_host
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(1, 1), (7, 3), (40, 17), (64, 64), (130, 257), (1001, 5)])
def test_place_host_has_the_strides_and_offsets_of_the_table(m, n, dtype):
    isz = np.dtype(dtype).itemsize
    per64 = 64 // isz
    want = {  # layout: (row stride, column stride, first row, first column, row step inside the parent)
        "mat": (1, -(-m // per64) * per64, 0, 0, 1),
        "sub": (1, 2 * m + 5, 5, 3, 1),
        "odd": (1, m + 3 if (m + 3) % 2 else m + 4, 1, 2, 1),
        "rowpad": (n + 3, 1, 2, 1, 1),
        "step2": (2, 2 * (m + 4), 1, 1, 2),
    }
    assert sorted(want) == sorted(LAYOUTS)
    a = np.arange(1, m * n + 1, dtype=dtype).reshape(m, n)
    for layout, (rs, cs, r0, c0, step) in want.items():
        parent, view = place_host(a, layout)
        box = view_box(a.shape, layout, dtype)
        assert view.shape == (m, n) and np.array_equal(view, a)
        assert (view.strides[0] // isz, view.strides[1] // isz) == (rs, cs) == (box.row_stride, box.col_stride)
        assert (box.r0, box.c0, box.rstep) == (r0, c0, step)
        ps = (parent.strides[0] // isz, parent.strides[1] // isz)
        assert (view.ctypes.data - parent.ctypes.data) // isz == r0 * ps[0] + c0 * ps[1]
        assert (rs, cs) == (ps[0] * step, ps[1])
        if layout == "mat":
            assert (cs * isz) % 64 == 0 and box.base == 0  # the view starts the allocation, every column on a 64-byte multiple of it
        if layout == "odd":
            assert cs % 2 == 1
        if layout in ("sub", "odd", "step2"):  # one element off every wider alignment, relative to the allocation
            off = box.base + r0 * ps[0] + c0 * ps[1]
            assert off % 2 == 1, (layout, off)
        # the view is never the end of the allocation, and the parent is dense: view + guard tile it without overlap
        assert sorted(ps) == [1, max(ps)] and max(ps) == parent.shape[0 if ps[0] == 1 else 1]
        last = (r0 + step * (m - 1)) * ps[0] + (c0 + n - 1) * ps[1]
        assert last < parent.size - 1
        mask = box.view_mask()
        assert mask.sum() == m * n and np.array_equal(parent[mask], a.ravel())
        assert (bits(parent)[~mask] == GUARD_BITS[isz]).all() and (~mask).sum() == parent.size - m * n
        assert np.isnan(guard_fill(dtype)) and not np.isnan(view).any()
        _, v2 = place_host(a, layout, fill=-7.5)
        assert np.array_equal(v2, a)


# ------------------------------------------------------------------------------------------------ the oracle on views
def _dense_like(a, layout):
    """a dense array of the major order of `layout` (row stride < column stride: column major)"""
    return np.array(a, order="C" if layout == "rowpad" else "F")


def _sym(rng, n, dtype):
    x = rng.standard_normal((n, n))
    return np.asarray(x + x.T, dtype=dtype)


def _spd(rng, n, dtype):
    x = rng.standard_normal((n, n))
    return np.asarray(x @ x.T + n * np.eye(n), dtype=dtype)


def _run_both(layout, mats, fn, dense_order=None):
    """fn(*arrays) on dense arrays and on views placed in `layout`: bit-identical arrays and return values, guards intact"""
    dense = [_dense_like(x, layout) if dense_order is None else np.array(x, order=dense_order) for x in mats]
    placed = [place_host(x, layout) for x in mats]
    before = [p.copy() for p, _ in placed]
    r_dense = fn(*dense)
    r_view = fn(*[v for _, v in placed])
    for x, (p, v), p0 in zip(dense, placed, before):
        assert np.array_equal(bits(np.ascontiguousarray(x)), bits(np.ascontiguousarray(v))), "factors differ between a dense array and a view"
        guard_intact(p, p0, view_box(x.shape, layout, x.dtype), "oracle")
    return r_dense, r_view


def _same_results(r_dense, r_view):
    assert len(r_dense) == len(r_view)
    for x, y in zip(r_dense, r_view):
        assert np.array_equal(x, y)


RECT = [(40, 17), (300, 200), (130, 257)]
SQUARE = [40, 130, 300]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", RECT)
def test_oracle_pivoted_factorizations_are_layout_stable(m, n, dtype, layout):
    """partial-pivot LU, full-pivot LU, column-pivot QR: same permutations, transposition counts and factor bits"""
    rng = np.random.default_rng(m * 3 + n)
    a = np.asarray(rng.standard_normal((m, n)), dtype=dtype)
    _same_results(*_run_both(layout, [a], lambda x: O.lu_in_place(x)))
    _same_results(*_run_both(layout, [a], lambda x: O.full_piv_lu_in_place(x)))
    size = min(m, n)
    bs = O.qr_recommended_block_size(m, n, dtype)
    h = np.zeros((bs, size), dtype=dtype)
    # the reference delays its rank-1 updates only for row stride 1 (qr/col_pivoting/factor.rs, `delayed_ok`): the dense array
    # that takes the path of a view with two non-unit strides is the row-major one.  The pivot search runs over columns either way
    order = "C" if layout == "step2" else None
    _same_results(*_run_both(layout, [a * np.logspace(0, -3, n).astype(dtype)[None, :], h], lambda x, t: O.colpiv_qr_in_place(x, t), order))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", RECT)
def test_oracle_qr_and_bidiag_are_layout_stable(m, n, dtype, layout):
    rng = np.random.default_rng(m * 5 + n)
    a = np.asarray(rng.standard_normal((m, n)), dtype=dtype)
    size = min(m, n)
    for bs in (4, 32):
        rd, rv = _run_both(layout, [a, np.zeros((bs, size), dtype=dtype)], lambda x, t: O.qr_in_place(x, t))
        assert rd == rv == size
    if m >= n:
        _run_both(layout, [a, np.zeros((8, n), dtype=dtype), np.zeros((5, n - 1), dtype=dtype)], lambda x, l, r: O.bidiag_in_place(x, l, r) and None)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SQUARE)
def test_oracle_symmetric_and_square_reductions_are_layout_stable(n, dtype, layout):
    """LLT, LDLT (with a sentinel strict upper triangle, which must stay), tridiagonalization, Hessenberg"""
    rng = np.random.default_rng(n)
    iu = np.triu_indices(n, 1)
    a = _spd(rng, n, dtype)
    a[iu] = -7.5
    rd, rv = _run_both(layout, [a], lambda x: O.llt_in_place(x))
    assert rd == rv == ("ok", 0)
    rd, rv = _run_both(layout, [a], lambda x: O.ldlt_in_place(x))
    assert rd == rv == ("ok", 0)
    bad = n // 2
    a[bad, bad] = -1.0
    rd, rv = _run_both(layout, [a], lambda x: O.llt_in_place(x))
    assert rd == rv == ("non_positive_pivot", bad)
    s = _sym(rng, n, dtype)
    s[iu] = -7.5
    _, v = place_host(s, layout)
    O.tridiag_in_place(v, np.zeros((8, n - 1), dtype=dtype, order="F"))
    assert (v[iu] == -7.5).all()
    _run_both(layout, [s, np.zeros((8, n - 1), dtype=dtype)], lambda x, t: O.tridiag_in_place(x, t) and None)
    g = np.asarray(rng.standard_normal((n, n)), dtype=dtype)
    _run_both(layout, [g, np.zeros((8, n - 1), dtype=dtype)], lambda x, t: O.hessenberg_in_place(x, t) and None)
    if n * n >= 256 * 256:
        _run_both(layout, [g, np.zeros((8, n - 1), dtype=dtype)], lambda x, t: O.hessenberg_blocked_in_place(x, t) and None)


# ------------------------------------------------------------------------------------------------ guard_intact
def _stray(layout, dtype, write):
    a = np.arange(1, 12 * 5 + 1, dtype=dtype).reshape(12, 5)
    parent, view = place_host(a, layout)
    box = view_box(a.shape, layout, dtype)
    before = parent.copy()
    write(parent, view, box)
    guard_intact(parent, before, box, "stand-in kernel")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_guard_intact_has_teeth(layout, dtype):
    def inside(parent, view, box):
        view[:] = -view
        view[3, 2] = np.nan

    _stray(layout, dtype, inside)  # writes inside the view are none of its business

    def below(parent, view, box):  # a ragged row tail rounded up to a full vector store
        parent[box.r0 + box.rstep * box.nrows, box.c0 + 1] = 1.0

    with pytest.raises(AssertionError, match=r"\(row 12, column 1\) in the padding below a column"):
        _stray(layout, dtype, below)

    def beyond(parent, view, box):  # one column too many
        parent[box.r0 + box.rstep * 4, box.c0 + box.ncols] = 2.0

    with pytest.raises(AssertionError, match=r"\(row 4, column 5\) beyond the last column"):
        _stray(layout, dtype, beyond)

    def payload(parent, view, box):  # the value is still "a NaN": only the bits tell
        isz = np.dtype(dtype).itemsize
        bits(parent)[box.r0 + box.rstep * box.nrows, box.c0] = GUARD_BITS[isz] ^ 1
        assert np.isnan(parent[box.r0 + box.rstep * box.nrows, box.c0])

    with pytest.raises(AssertionError, match=r"\(row 12, column 0\) in the padding below a column"):
        _stray(layout, dtype, payload)

    def plain_nan(parent, view, box):  # a computed NaN written over the guard NaN
        parent[box.r0 + box.rstep * box.nrows, box.c0 + 4] = np.nan

    with pytest.raises(AssertionError, match="1 element"):
        _stray(layout, dtype, plain_nan)

    if layout == "step2":
        def between(parent, view, box):  # addressed with row stride 1 instead of the view's
            parent[box.r0 + 1, box.c0] = 3.0

        with pytest.raises(AssertionError, match=r"\(row 0\+1/2, column 0\) between two rows of the view"):
            _stray(layout, dtype, between)
    if box_has_rows_above(layout):
        def above(parent, view, box):
            parent[box.r0 - 1, box.c0] = 4.0

        with pytest.raises(AssertionError, match=r"column 0\) in the padding above a column"):
            _stray(layout, dtype, above)


def box_has_rows_above(layout):
    return view_box((12, 5), layout, np.float64).r0 > 0


def test_guard_intact_reports_the_first_few_of_many():
    a = np.ones((12, 5))
    parent, view = place_host(a, "sub")
    box = view_box(a.shape, "sub", np.float64)
    before = parent.copy()
    parent[:] = 0.0  # i + j * nrows addressing gone wild
    with pytest.raises(AssertionError) as ei:
        guard_intact(parent, before, box)
    assert f"{parent.size - 60} element(s) outside the 12 x 5 view changed" in str(ei.value)
    assert str(ei.value).count("->") == 8
