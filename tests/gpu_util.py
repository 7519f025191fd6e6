"""helpers shared by the -m gpu parity tests (device tensors are column major like faer::Mat)."""
import contextlib
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

EPS = {np.dtype(np.float64): np.finfo(np.float64).eps, np.dtype(np.float32): np.finfo(np.float32).eps}


def fa():
    return ge.load_package()


def init_gpu():
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    m = fa()
    m.lib()
    m.use_torch_stream()
    return m


def to_dev(x, order="F"):
    """numpy 2-D array -> torch cuda tensor with the requested memory order (same logical values)."""
    import torch

    x = np.asarray(x)
    if order == "F":
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(t):
    fa().synchronize()
    return t.detach().cpu().numpy()


def rnd(rng, m, n, dtype=np.float64, order="F"):
    return np.asarray(rng.standard_normal((m, n)), dtype=dtype, order=order)


def spd(rng, n, dtype=np.float64):
    a = rng.standard_normal((n, n))
    return np.asarray(a @ a.T + n * np.eye(n), dtype=dtype, order="F")


def sym(rng, n, dtype):
    a = rng.standard_normal((n, n))
    return np.asarray(a + a.T, dtype=dtype, order="F")


def well_conditioned(rng, n, dtype):
    return np.asarray(rng.standard_normal((n, n)) + 2 * np.sqrt(n) * np.eye(n), dtype=dtype, order="F")


def quasi_definite(rng, n, dtype=np.float64):
    n1 = n // 2
    h = rng.standard_normal((n, n))
    H = h[:n1, :n1] @ h[:n1, :n1].T + n * np.eye(n1)
    G = h[n1:, n1:] @ h[n1:, n1:].T + n * np.eye(n - n1)
    B = h[n1:, :n1]
    return np.asarray(np.block([[H, B.T], [B, -G]]), dtype=dtype, order="F"), n1


def boosted(n):
    """positive definite with its largest diagonal entry at index 0, so that step 0 of a diagonally pivoted factorization does not swap"""
    import piv_llt_ref

    a = piv_llt_ref.spd(n, 3 + n)
    a[0, 0] = 2 * np.diag(a).max()
    return a


# ---- bit patterns (NaN payloads and signed zeros compare as what they are)
def bits(t):
    """the elements of a torch tensor or numpy array as integers of the same width"""
    if isinstance(t, np.ndarray):
        return t.view(np.int64 if t.dtype == np.float64 else np.int32)
    import torch

    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(x, y):
    import torch

    return torch.equal(bits(x.contiguous()), bits(y.contiguous()))


# ---- padded and offset views inside a guarded parent (the forms faer hands device matrices over in)
LAYOUTS = ("mat", "sub", "odd", "rowpad", "step2")
# quiet NaNs with a payload no computation produces; built from integers and compared through integer views only
GUARD_BITS = {8: 0x7FF8DEADBEEF0BAD, 4: 0x7FC0BEEF}


def guard_fill(dtype):
    dt = np.dtype(dtype)
    return np.array([GUARD_BITS[dt.itemsize]], dtype=np.int64 if dt.itemsize == 8 else np.int32).view(dt)[0]


class ViewBox:
    """where a view sits in its parent, all in elements: the parent is a `shape` array with element strides `pstrides`, stored
    `base` elements into its allocation; view (i, j) is parent (r0 + i * rstep, c0 + j)"""

    def __init__(self, nrows, ncols, layout, isz):
        self.nrows, self.ncols, self.layout, self.rstep, self.base = nrows, ncols, layout, 1, 0
        if layout == "mat":  # faer::Mat: columns padded to 64 bytes, the allocation itself aligned
            ld = -(-max(nrows, 1) // (64 // isz)) * (64 // isz)
            self.r0, self.c0, self.shape, self.pstrides = 0, 0, (ld, ncols + 2), (1, ld)
        elif layout == "sub":  # a block of a bigger column-major matrix, which itself starts one element into its allocation
            ld = 2 * nrows + 5  # (row 5, column 3 of such a parent alone is an even element offset: 16-byte aligned in fp64)
            self.r0, self.c0, self.shape, self.pstrides, self.base = 5, 3, (ld, ncols + 5), (1, ld), 1
        elif layout == "odd":  # odd column stride: every column aligned to one element only
            ld = nrows + 3 + (nrows % 2)
            self.r0, self.c0, self.shape, self.pstrides = 1, 2, (ld, ncols + 4), (1, ld)
        elif layout == "rowpad":  # row-major parent with padded rows
            ld = ncols + 3
            self.r0, self.c0, self.shape, self.pstrides = 2, 1, (nrows + 4, ld), (ld, 1)
        elif layout == "step2":  # every second row of a column-major parent: both strides non-unit
            ld = 2 * (nrows + 4)
            self.r0, self.c0, self.shape, self.pstrides, self.rstep = 1, 1, (ld, ncols + 2), (1, ld), 2
        else:
            raise ValueError(layout)
        self.row_stride, self.col_stride = self.pstrides[0] * self.rstep, self.pstrides[1]
        self.numel = self.shape[0] * self.shape[1]  # the parent is dense in its own order

    def rows(self):
        return slice(self.r0, self.r0 + self.rstep * self.nrows, self.rstep)

    def cols(self):
        return slice(self.c0, self.c0 + self.ncols)

    def view_mask(self):
        m = np.zeros(self.shape, bool)
        m[self.rows(), self.cols()] = True
        return m


def view_box(shape, layout, dtype):
    return ViewBox(shape[0], shape[1], layout, np.dtype(dtype).itemsize)


def _place_flat(a, layout, fill):
    a = np.asarray(a)
    assert a.ndim == 2 and a.dtype in (np.float64, np.float32)
    box = view_box(a.shape, layout, a.dtype)
    flat = np.empty(box.base + box.numel, dtype=a.dtype)
    flat[:] = guard_fill(a.dtype) if fill is None else fill
    parent = np.lib.stride_tricks.as_strided(flat[box.base:], box.shape, tuple(s * a.itemsize for s in box.pstrides))
    parent[box.rows(), box.cols()] = a
    return box, flat, parent


def place_host(a, layout, fill=None):
    """(parent, view) as numpy arrays: `view` holds the values of `a` with the element strides of `layout`, every other element
    of `parent` is `fill` (default: the guard NaN)"""
    box, _, parent = _place_flat(a, layout, fill)
    return parent, parent[box.rows(), box.cols()]


def place(a, layout, fill=None):
    """place_host on the device: (parent, view) as torch cuda tensors with the same element strides"""
    import torch

    box, flat, _ = _place_flat(a, layout, fill)
    dev = torch.from_numpy(bits(flat)).cuda().view(torch.float64 if flat.dtype == np.float64 else torch.float32)
    parent = dev.as_strided(box.shape, box.pstrides, box.base)
    return parent, parent[box.rows(), box.cols()]


def _host_bits(t):
    return np.array(bits(t) if isinstance(t, np.ndarray) else bits(t).cpu().numpy())


def guard_intact(parent, parent0, box, what=""):
    """every element of `parent` outside the view has the bit pattern it has in the snapshot `parent0`; otherwise an
    AssertionError names the first changed coordinates relative to the view and the kind of padding they lie in"""
    now, was = _host_bits(parent), _host_bits(parent0)
    assert now.shape == was.shape == tuple(box.shape)
    bad = np.argwhere((now != was) & ~box.view_mask())
    if len(bad) == 0:
        return
    lines = []
    for pr, pc in bad[:8]:
        i, rem = divmod(int(pr) - box.r0, box.rstep)
        j = int(pc) - box.c0
        if j >= box.ncols:
            where = "beyond the last column"
        elif j < 0:
            where = "before the first column"
        elif i >= box.nrows:
            where = "in the padding below a column"
        elif i < 0:
            where = "in the padding above a column"
        else:
            assert rem != 0
            where = "between two rows of the view"
        row = f"{i}" if rem == 0 else f"{i}+{rem}/{box.rstep}"
        lines.append(f"(row {row}, column {j}) {where}: {int(was[pr, pc]):#x} -> {int(now[pr, pc]):#x}")
    raise AssertionError(f"{what} layout {box.layout}: {len(bad)} element(s) outside the {box.nrows} x {box.ncols} view changed; first: "
                         + "; ".join(lines))


# ---- route counters of the GEMM / TRSM dispatch (faer_hip_debug_route_counts)
def route_names():
    """FaerHipRoute_* in enum order, read from the header (like test_cabi.py reads the exports)"""
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    vals = {int(v): k for k, v in re.findall(r"FaerHipRoute_(\w+)\s*=\s*(\d+)", hdr) if k != "Count"}
    assert sorted(vals) == list(range(len(vals)))
    return [vals[i] for i in range(len(vals))]


ROUTES = route_names()


class Routes:
    """with Routes(F) as r: ...  -- r.hits: {route name: launches} of the calls inside (this thread)"""

    def __init__(self, F):
        self.F = F
        self.lib = F.lib()
        self.lib.faer_hip_debug_route_counts.restype = C.c_size_t

    def __enter__(self):
        self.F.synchronize()
        self.lib.faer_hip_debug_route_reset()
        return self

    def __exit__(self, *exc):
        self.F.synchronize()
        buf = (C.c_longlong * len(ROUTES))()
        assert self.lib.faer_hip_debug_route_counts(buf, len(ROUTES)) == len(ROUTES)
        self.hits = dict(zip(ROUTES, buf))
        return False

    def assert_hit(self, *names):
        missing = [r for r in names if self.hits[r] <= 0]
        assert not missing, (missing, {k: v for k, v in self.hits.items() if v})


# ---- a non-blocking caller stream and the ordering protocol of tests/test_gpu_stream_order.py
DELAY_PRODUCTS = 12  # 4096^3 fp64 products of delay(): about 1.9 ms each at the README's 72 TFLOP/s; sized by the module's control
_DELAY_OPERANDS = []


@contextlib.contextmanager
def on_stream(S):
    """torch's current stream and the library's stream are the non-blocking `S` inside, the default stream again afterwards"""
    import torch

    F = fa()
    assert S.cuda_stream != 0
    try:
        with torch.cuda.stream(S):
            F.use_torch_stream()
            yield S
    finally:
        F.use_torch_stream()  # (torch is back on its default stream here)


def delay_operands():
    """the operands of delay(), allocated and filled on the default stream: call it before the host wait that precedes delay()"""
    import torch

    if not _DELAY_OPERANDS:
        g = torch.Generator(device="cuda").manual_seed(1)
        _DELAY_OPERANDS.extend(torch.rand((4096, 4096), dtype=torch.float64, device="cuda", generator=g).t() for _ in range(2))
        _DELAY_OPERANDS.append(torch.zeros((4096, 4096), dtype=torch.float64, device="cuda").t())
    return _DELAY_OPERANDS


def delay(S, products=DELAY_PRODUCTS):
    """keeps `S` busy with the library's own DGEMM (inside on_stream(S)); the host does not wait"""
    import torch

    F = fa()
    assert _DELAY_OPERANDS, "delay_operands() first"
    assert torch.cuda.current_stream() == S and F.lib().faer_hip_get_stream() == S.cuda_stream
    a, b, c = _DELAY_OPERANDS
    for _ in range(products):
        F.matmul(c, F.ACCUM_REPLACE, a, b, 1.0)


def _fresh(src):
    """device copies with the memory order of the source (a C-contiguous numpy matrix stays row major)"""
    def one(v):
        if not isinstance(v, np.ndarray):
            return v.clone()
        return to_dev(v, "C" if v.flags.c_contiguous and not v.flags.f_contiguous else "F")

    return {k: one(v) for k, v in src.items()}


def _host(out):
    import torch

    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def ordered_call(fn, inputs_good, inputs_stale, S=None, products=DELAY_PRODUCTS, routes=()):
    """`fn(bufs)` runs public calls on the device tensors `bufs` (one per entry of the inputs: numpy arrays or device tensors of the
    same shapes) and returns {name: device tensor or host value}.  Returns (expected, got) as host values:
    expected -- fn on fresh copies of inputs_good on the default stream, synchronised;
    got      -- the working buffers hold inputs_stale; then on the non-blocking stream S, with no host synchronisation in between:
                delay, the copy of inputs_good into the buffers (the producer), fn, a copy of every output tensor (the consumer);
                the host waits for S alone.
    A call that starts before the producer factors the stale matrix; a call whose internal streams have not been joined into S
    when it returns leaves unfinished outputs to the consumer.  `routes`: dispatch routes the expected run must hit."""
    import torch

    F = fa()
    assert inputs_good.keys() == inputs_stale.keys()
    with Routes(F) as r:
        first = fn(_fresh(inputs_good))
    r.assert_hit(*routes)  # the GEMM / TRSM dispatch routes the case is about (the same inputs take them again on S)
    expected = _host(first)
    good, bufs = _fresh(inputs_good), _fresh(inputs_stale)
    snaps = {k: torch.empty_like(v) for k, v in first.items() if torch.is_tensor(v)}
    delay_operands()
    S = S or torch.cuda.Stream()
    torch.cuda.synchronize()  # S is non-blocking: it would not wait for the fills above
    with on_stream(S):
        delay(S, products)
        for k in bufs:
            bufs[k].copy_(good[k], non_blocking=True)
        out = fn(bufs)
        for k in snaps:
            snaps[k].copy_(out[k], non_blocking=True)
    S.synchronize()  # that stream only
    got = _host({k: (snaps[k] if k in snaps else v) for k, v in out.items()})
    del first, good, bufs, snaps, out  # (alive until here: allocated on the default stream, used on S)
    return expected, got


def same_result(expected, got, what=""):
    """every entry bit for bit (floating point) or exactly (indices, counts, status)"""
    assert expected.keys() == got.keys(), (what, sorted(expected), sorted(got))
    for k, e in expected.items():
        g = got[k]
        if isinstance(e, np.ndarray):
            assert e.dtype == g.dtype and e.shape == g.shape, (what, k)
            if e.dtype.kind == "f":
                ne = bits(np.ascontiguousarray(e)) != bits(np.ascontiguousarray(g))
                assert not ne.any(), (what, k, f"{int(ne.sum())} of {ne.size} entries differ; first at {tuple(np.argwhere(ne)[0])}")
            else:
                assert np.array_equal(e, g), (what, k)
        else:
            assert e == g, (what, k, e, g)
