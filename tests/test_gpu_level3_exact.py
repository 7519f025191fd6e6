"""Exact-integer pins of every GEMM and TRSM route (csrc/gemm.hip gemm_dev, csrc/trsm.hip trsm_lower_dev / trsm_rec).

Every operand entry, alpha, the diagonals and C0 are dyadic numbers whose products and partial sums fit the mantissa of the
test dtype: small integers, powers of two for alpha and the diagonals.  The result is then exact in any summation order --
with or without FMA, split-K or a fused epilogue -- and every route must match the exact answer BIT FOR BIT in both
precisions (the f32 MFMA of gfx950 computes exact fp32 products; it has no reduced-precision form).  References are plain
fp64 products of the same integer data, exact as well.  Each GEMM row names the route it pins; the test asserts that the
route's counter (faer_hip_debug_route_counts) went up, so a dispatch change cannot silently move a row to another kernel.

The CPU tests at the end check that the case tables name every route of include/faer_hip.h (or list it in DRIVER_ONLY with
the test that reaches it) and that the exactness budget agrees with Python integer arithmetic."""
import ctypes as C
import itertools
import os
import re
import zlib
from fractions import Fraction

import numpy as np
import pytest

from gpu_util import ROOT, ROUTES, Routes, bits, init_gpu, same_bits

F32, F64 = np.float32, np.float64
DTYPES = [F64, F32]
MANT = {np.dtype(F32): 24, np.dtype(F64): 53}
# integer range of operand entries: fp64 products reach 2^24, so a kernel that accumulated fp64 data in fp32 would round
RANGE = {np.dtype(F32): 15, np.dtype(F64): 4095}


# ------------------------------------------------------------------------------------------------ route counters
# routes no direct call reaches: only the factorization drivers issue them (or nothing does), with the test that covers them
# (slots of routes that were removed with their kernels stay in the enum, named Retired<slot>: they always count zero)
RETIRED = [r for r in ROUTES if r.startswith("Retired")]
LEVEL2_ROUTES = ("GemmZeroK", "GemmRank1", "GemmGemv", "GemmSkinny")
DRIVER_ONLY = {
    "GemmTriSkipSplit": "tests.test_gpu_factor::test_llt_lookahead_on_a_view_with_reversed_rows_and_columns",
    "TrsmLeafPacked16": "tests.test_gpu_factor::test_llt_vs_oracle",
    "TrsmLeafPacked32": "tests.test_gpu_factor::test_llt_full_size_property",
}


# ------------------------------------------------------------------------------------------------ generator
def frac_bits(values):
    """fractional bits of the dyadic numbers in `values` (finite entries only)"""
    x = np.abs(np.asarray(values, dtype=np.float64).ravel())
    x = x[np.isfinite(x)]
    for b in range(64):
        y = x * 2.0 ** b
        if np.array_equal(y, np.floor(y)):
            return b
    raise AssertionError("not dyadic")


def exact_budget(dtype, k, amax, bmax, alpha=1.0, c0max=0.0, dmax=1.0, frac=0):
    """largest magnitude (in units of 2^-frac) any partial sum of [C0 +] alpha * A diag B can take, next to the dtype's
    mantissa: every partial sum of the accumulators (|.| <= k max|A| max|d| max|B|, from -C0 / C0 in the fused epilogues)
    and the result are exact iff this stays below 2^p"""
    s = float(k) * amax * dmax * bmax
    mag = max(1.0, abs(alpha)) * s + c0max
    units = mag * 2.0 ** frac
    return units, 2.0 ** MANT[np.dtype(dtype)]


def assert_exact_budget(dtype, k, a=None, b=None, alpha=1.0, c0=None, diag=None, amax=None, bmax=None):
    """asserts on the host, before a call, that the case stays inside the exact range (a, b, c0, diag: numpy or torch)"""
    def mx(t):
        if t is None:
            return 0.0
        if hasattr(t, "detach"):
            import torch

            t = t.detach()
            f = t[torch.isfinite(t)]
            return float(f.abs().max().item()) if f.numel() else 0.0
        t = np.asarray(t, dtype=np.float64)
        t = t[np.isfinite(t)]
        return float(np.abs(t).max()) if t.size else 0.0

    def fb(t):
        if t is None:
            return 0
        if hasattr(t, "detach"):
            t = t.detach().double()
            t = t[t.isfinite()].unique().cpu().numpy()  # (few distinct values: small integers)
        return frac_bits(t)

    amax = mx(a) if amax is None else amax
    bmax = mx(b) if bmax is None else bmax
    dmax = mx(diag) if diag is not None else 1.0
    frac = max(fb(a) + fb(b) + fb(diag) + frac_bits([alpha]), fb(c0))
    units, lim = exact_budget(dtype, k, amax, bmax, alpha, mx(c0), dmax, frac)
    assert units < lim, f"case leaves the exact range: {units:.3g} >= 2^{MANT[np.dtype(dtype)]}"


def ints(g, shape, r, dtype, order="F", device="cuda"):
    """integer entries in [-r, r] as a device tensor of `dtype`, column major (F) or row major (C)"""
    import torch

    tdt = torch.float64 if dtype == F64 else torch.float32
    rows, cols = shape
    if order == "F":
        t = torch.randint(-r, r + 1, (cols, rows), generator=g, device=device, dtype=torch.int64).to(tdt).t()
    else:
        t = torch.randint(-r, r + 1, (rows, cols), generator=g, device=device, dtype=torch.int64).to(tdt)
    return t


def tdtype(dtype):
    import torch

    return torch.float64 if dtype == F64 else torch.float32


def suffix(dtype):
    return "f64" if dtype == F64 else "f32"


# ------------------------------------------------------------------------------------------------ GEMM case table
# (route, m, n, k, layouts of A B C, accum, alpha, dst kind, extras, further routes the row must hit)
GEMM_ROWS = [
    # level-2 and degenerate shapes
    ("GemmZeroK", 17, 15, 0, "FFF", "replace", 2.0, "full", "", ()),
    ("GemmZeroK", 16, 16, 0, "FFF", "add", -1.0, "lower", "", ()),
    ("GemmRank1", 65, 129, 1, "FFF", "replace", 2.0, "full", "", ()),
    ("GemmRank1", 1, 1, 1, "CCF", "add", -0.5, "full", "", ()),
    ("GemmGemv", 129, 1, 1025, "FFF", "add", -0.5, "full", "", ()),
    ("GemmGemv", 1, 63, 17, "CFF", "replace", 1.0, "full", "", ()),
    ("GemmGemv", 1, 1, 1023, "FCF", "add", 1.0, "full", "", ()),
    ("GemmSkinny", 20001, 30, 16, "FFF", "add", -1.0, "full", "", ()),
    # ragged tile edges on the pipelined 64 x 64 tile (k 1023 .. 1025: 1024 and up split along K)
    ("GemmPipe64", 15, 17, 16, "FFF", "replace", 1.0, "full", "", ()),
    # (a column-major rhs with fewer than 16 rows: the descriptor-addressed B loader cannot take it, the pointer loaders do)
    ("GemmLegacy64", 16, 16, 15, "CFF", "add", -0.5, "full", "", ()),
    ("GemmPipe64", 17, 15, 17, "FCF", "add", 1.0, "full", "", ()),
    ("GemmPipe64", 63, 65, 1023, "CCF", "add", -1.0, "full", "", ()),
    ("GemmPipe64", 64, 127, 17, "FFF", "replace", 2.0, "full", "", ()),
    ("GemmPipe64", 127, 129, 1023, "FFF", "add", -0.5, "full", "", ()),
    ("GemmPipe64", 128, 128, 16, "CCF", "replace", 1.0, "full", "", ()),
    ("GemmPipe64", 65, 63, 15, "FCF", "add", 1.0, "full", "", ()),
    ("GemmSplitK", 129, 127, 1025, "FFF", "add", -0.5, "full", "", ()),
    ("GemmSplitK", 64, 64, 1024, "CFF", "replace", 2.0, "full", "", ()),
    ("GemmSplitK", 17, 63, 1025, "FCF", "add", 1.0, "full", "", ()),
    # split-K FULL (ragged last slice)
    ("GemmSplitK", 300, 300, 5000, "FFF", "add", -0.5, "full", "", ()),
    ("GemmSplitK", 300, 300, 5001, "FFF", "replace", 2.0, "full", "", ()),
    ("GemmSplitK", 300, 300, 5001, "CCF", "add", 1.0, "full", "", ()),
    ("GemmSplitK", 2047, 100, 1030, "FFF", "add", -1.0, "full", "", ()),
    # split-K with a triangular dst: Lower, Upper (through the transposition), strict Lower / Upper
    ("GemmSplitK", 300, 300, 4099, "FFF", "add", -1.0, "lower", "", ("GemmTriEnum",)),
    ("GemmSplitK", 300, 300, 4099, "FFF", "replace", 2.0, "lower", "", ("GemmTriEnum",)),
    ("GemmSplitK", 300, 300, 4099, "FFF", "add", -0.5, "upper", "", ("GemmTransposed", "GemmTriEnum")),
    ("GemmSplitK", 300, 300, 4099, "FFF", "add", 1.0, "strict_lower", "", ("GemmTriEnum",)),
    ("GemmSplitK", 300, 300, 4099, "CFF", "replace", 2.0, "strict_upper", "", ("GemmTransposed",)),
    ("GemmSplitK", 257, 200, 4099, "FFF", "add", -0.5, "lower", "", ()),  # lower, not square: no tile enumeration
    # structured lhs with split-K (the TRMM of a 2048 x 2048 triangle with 40 right-hand sides): slices that are empty
    # for a tile must still write zeros to the workspace
] + [("GemmExtra64", 2048, 40, 2048, "FFF", acc, al, "full", "astruct:" + s, ("GemmSplitK",))
     for s, acc, al in [("lower", "add", -1.0), ("upper", "replace", 2.0), ("strict_lower", "add", 1.0),
                        ("strict_upper", "replace", 1.0), ("unit_lower", "add", -0.5), ("unit_upper", "add", -1.0)]] + [
    ("GemmExtra64", 40, 2048, 2048, "FFF", "add", -1.0, "full", "bstruct:upper", ("GemmSplitK",)),
    # diag scaling, shallow and deep K
    ("GemmExtra64", 129, 65, 70, "FFF", "add", -0.5, "full", "diag", ()),
    ("GemmExtra64", 100, 90, 3000, "CFF", "replace", 1.0, "full", "diag", ("GemmSplitK",)),
    # index scatter (u32 / u64, device arrays), several tiles, Full and Lower dst: the pipelined kernel's general epilogue,
    # or the 64 x 64 extra kernel's with diag scaling
    ("GemmPipe64", 150, 150, 70, "FFF", "add", 1.0, "full", "idx32", ()),
    ("GemmPipe64", 150, 130, 70, "FFF", "replace", 2.0, "full", "idx64", ()),
    ("GemmExtra64", 150, 150, 70, "FFF", "add", -1.0, "lower", "idx32+diag", ("GemmTriEnum",)),
    ("GemmExtra64", 150, 130, 70, "CFF", "replace", 2.0, "full", "idx64+diag", ()),
    ("GemmPipe64", 150, 150, 70, "FFF", "add", -0.5, "lower", "idx64", ("GemmTriEnum",)),
    # the big tiles, naturally: 128 x 128 from 256 tiles, 128 x 256 for deep-K products with >= 512 of them
    ("GemmPipe128", 2048, 2048, 64, "FFF", "add", -1.0, "full", "", ("GemmFastIo3",)),
    ("GemmPipe128", 2944, 2944, 64, "FFF", "add", -0.5, "lower", "", ("GemmTriEnum",)),
    ("GemmPipeWide", 4096, 4096, 2048, "FFF", "replace", 1.0, "full", "", ("GemmFastIo1",)),
    # every forced variant (faer_hip_set_gemm_variant, process wide: restored in `finally`)
    ("GemmPipe128", 129, 127, 1023, "FFF", "add", 1.0, "full", "variant:1", ()),
    ("GemmPipe64", 2048, 2048, 64, "FFF", "replace", 2.0, "full", "variant:2", ()),
    ("GemmPipeWide", 300, 500, 70, "FFF", "add", -0.5, "full", "variant:3", ()),
    ("GemmPipeWide", 640, 640, 16, "FFF", "add", 1.0, "lower", "variant:3", ("GemmTriEnum",)),
    ("GemmPipeWide", 513, 513, 4099, "FFF", "add", -1.0, "lower", "variant:3", ("GemmSplitK", "GemmTriEnum")),
    ("GemmPipe128", 4096, 4096, 2048, "FFF", "add", 1.0, "full", "variant:5", ("GemmFastIo2",)),
    ("GemmPipe128", 128, 1024, 2048, "FFF", "add", -0.5, "full", "variant:6", ("GemmSplitK",)),
    ("GemmLegacy128", 129, 127, 100, "FFF", "add", -0.5, "full", "variant:11", ()),
    ("GemmLegacy128", 300, 300, 4099, "FFF", "add", 1.0, "lower", "variant:11", ("GemmSplitK", "GemmTriEnum")),
    ("GemmLegacy64", 129, 127, 100, "CCF", "replace", 2.0, "full", "variant:12", ()),
    ("GemmLegacy64", 300, 300, 5001, "FFF", "add", -1.0, "upper", "variant:12", ("GemmSplitK", "GemmTransposed")),
    # the non-pipelined fallback without a variant: negative strides, a leading dimension beyond the 32-bit offsets
    ("GemmLegacy64", 200, 130, 150, "FFF", "replace", 1.0, "full", "neg_strides", ()),
    ("GemmLegacy64", 24, 20, 100, "FFF", "add", -0.5, "full", "huge_ld", ()),
    # row-major dst: the product runs on dst^T
    ("GemmTransposed", 200, 300, 100, "FFC", "add", -0.5, "full", "", ("GemmPipe64",)),
    ("GemmTransposed", 130, 70, 1030, "CCC", "replace", 2.0, "full", "", ("GemmSplitK",)),
    # fused epilogues next to edge and diagonal tiles in the same launch: Replace alpha 1 / 2 into NaN, Add alpha 1 / -1
    # (fused), -0.5 (general); a ragged Full dst and a Lower dst with several tile rows
    ("GemmFastIo1", 200, 300, 100, "FFF", "replace", 1.0, "full", "", ("GemmPipe64",)),
    ("GemmFastIo1", 200, 300, 100, "CFF", "replace", 2.0, "full", "", ()),
    ("GemmFastIo1", 400, 400, 70, "FFF", "replace", 2.0, "lower", "", ("GemmTriEnum",)),
    ("GemmFastIo2", 200, 300, 100, "FFF", "add", 1.0, "full", "", ()),
    ("GemmFastIo2", 400, 400, 70, "FCF", "add", 1.0, "lower", "", ("GemmTriEnum",)),
    ("GemmFastIo3", 200, 300, 100, "CFF", "add", -1.0, "full", "", ()),
    ("GemmFastIo3", 400, 400, 70, "FFF", "add", -1.0, "lower", "", ("GemmTriEnum",)),
    ("GemmFastIo3", 400, 400, 70, "FFF", "add", -1.0, "strict_lower", "", ("GemmTriEnum",)),
    ("GemmPipe64", 400, 400, 70, "FFF", "add", -0.5, "lower", "", ("GemmTriEnum",)),
    # a dst view inside a sentinel-filled parent
    ("GemmFastIo2", 200, 150, 90, "FFF", "add", 1.0, "full", "parent", ()),
    ("GemmFastIo1", 200, 150, 90, "FFF", "replace", 2.0, "full", "parent", ()),
    ("GemmPipe64", 200, 150, 90, "FFF", "add", -0.5, "lower", "parent", ()),
]
GEMM_CASES = [(dt,) + row for row in GEMM_ROWS for dt in DTYPES]


def _gemm_id(c):
    dt, route, m, n, k, lay, acc, al, kind, extra = c[:10]
    return f"{suffix(dt)}-{route}-{m}x{n}x{k}-{lay}-{acc}{al:g}-{kind}" + (f"-{extra}" if extra else "")


def _dense(t, s):
    """the matrix an operand with FaerBlock `s` stands for (its other entries may hold anything, NaN included)"""
    import torch

    if s == "rect":
        return t
    z = torch.nan_to_num(t, nan=0.0)
    eye = torch.eye(t.shape[0], dtype=t.dtype, device=t.device)
    return {"lower": lambda: torch.tril(z), "upper": lambda: torch.triu(z), "strict_lower": lambda: torch.tril(z, -1),
            "strict_upper": lambda: torch.triu(z, 1), "unit_lower": lambda: torch.tril(z, -1) + eye,
            "unit_upper": lambda: torch.triu(z, 1) + eye}[s]()


def _mask(m, n, s, device="cuda"):
    """entries an operand / dst with FaerBlock `s` consists of (unit structures: the strict part; the diagonal is implied)"""
    import torch

    i = torch.arange(m, device=device)[:, None]
    j = torch.arange(n, device=device)[None, :]
    return {"rect": (i >= 0) & (j >= 0), "full": (i >= 0) & (j >= 0), "lower": i >= j, "upper": i <= j, "strict_lower": i > j,
            "strict_upper": i < j, "unit_lower": i > j, "unit_upper": i < j}[s]


def _nan_outside(t, s):
    """t with NaN in every entry a FaerBlock-`s` operand must not read (for unit / strict structures: the diagonal too)"""
    import torch

    if s == "rect":
        return t
    v = t.clone()
    v[~_mask(t.shape[0], t.shape[1], s, t.device)] = float("nan")
    return v


def gemm_row_problem(dtype, row):
    """the inputs of faer_hip_debug_gemm_plan (faer_rs_amd.GEMM_PLAN_INPUTS) for the library call test_gemm_route_is_exact makes
    for a row of GEMM_ROWS: its shapes and options and the element strides of the operands the test builds (the test asserts
    that its tensors have them).  No GPU needed."""
    route, m, n, k, lay, acc, alpha, kind, extra, more = row
    extras = dict(e.split(":") if ":" in e else (e, "") for e in extra.split("+") if e)
    block = {"rect": 0, "lower": 1, "upper": 2, "strict_lower": 3, "strict_upper": 4, "unit_lower": 5, "unit_upper": 6}
    indexed = "idx32" in extras or "idx64" in extras
    dm, dn = (m + 250, n + 250) if indexed else (m, n)
    ars, acs = (1, m) if lay[0] == "F" else (k, 1)
    brs, bcs = (1, k) if lay[1] == "F" else (n, 1)
    drs, dcs = (1, dm + 9) if "parent" in extras else (1, dm) if lay[2] == "F" else (dn, 1)
    if "neg_strides" in extras:
        ars, bcs = -ars, -bcs
    if "huge_ld" in extras:
        brs, bcs = 1, (1 << 31) // (256 * np.dtype(dtype).itemsize) + 1000
    return dict(m=m, n=n, k=k, elem_bytes=np.dtype(dtype).itemsize, kind={"f": 0, "l": 1, "u": 2}[kind.replace("strict_", "")[0]],
                add=int(acc == "add"), alpha_sign={1.0: 1, -1.0: -1}.get(alpha, 0), drs=drs, dcs=dcs, ars=ars, acs=acs, brs=brs, bcs=bcs,
                indexed=int(indexed), diag=int("diag" in extras), a_struct=block[extras.get("astruct", "rect")],
                b_struct=block[extras.get("bstruct", "rect")], variant=int(extras.get("variant", 0)))


def _set_variant(F, v):
    F.lib().faer_hip_set_gemm_variant(C.c_int(v))


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=_gemm_id)
def test_gemm_route_is_exact(case):
    import torch

    dtype, route, m, n, k, lay, acc, alpha, kind, extra, more = case
    F = init_gpu()
    tdt = tdtype(dtype)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(_gemm_id(case).encode()))
    r = RANGE[np.dtype(dtype)]
    add = acc == "add"
    extras = dict(e.split(":") if ":" in e else (e, "") for e in extra.split("+") if e)
    astruct, bstruct = extras.get("astruct", "rect"), extras.get("bstruct", "rect")
    a = ints(g, (m, k), r, dtype, lay[0])
    b = ints(g, (k, n), r, dtype, lay[1])
    diag = None
    if "diag" in extras:
        pw = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=tdt, device="cuda")
        diag = pw[torch.randint(0, 6, (k,), generator=g, device="cuda")]
    ri = ci = None
    if "idx32" in extras or "idx64" in extras:
        it = torch.int32 if "idx32" in extras else torch.int64
        dm, dn = m + 250, n + 250
        sel = torch.sort(torch.randperm(dm, generator=g, device="cuda")[:m]).values
        ri = sel.to(it)
        ci = (sel if kind == "lower" else torch.randperm(dn, generator=g, device="cuda")[:n]).to(it)
    else:
        dm, dn = m, n
    # dst: C0 integers (Add) or NaN (Replace: never read); for a triangular dst the other part must survive bit for bit
    c0 = ints(g, (dm, dn), r, dtype, lay[2]) if add else torch.full((dm, dn), float("nan"), dtype=tdt, device="cuda")
    parent = None
    if "parent" in extras:
        parent = torch.full((dm + 9, dn + 11), -7.75, dtype=tdt, device="cuda").t().contiguous().t()
        parent[0, 0] = float("nan")
        parent[3:3 + dm, 5:5 + dn] = c0
        dst = parent[3:3 + dm, 5:5 + dn]
        parent0 = parent.clone()
    elif lay[2] == "C":
        dst = c0.contiguous().clone()
    else:
        dst = torch.empty_strided((dm, dn), (1, dm), dtype=tdt, device="cuda").copy_(c0)
    # exact reference (fp64, exact for integer data in any order)
    a64, b64 = _dense(a.double(), astruct), _dense(b.double(), bstruct)
    if diag is not None:
        a64 = a64 * diag.double()[None, :]
    prod = alpha * (a64 @ b64) if k > 0 else torch.zeros((m, n), dtype=torch.float64, device="cuda")
    assert_exact_budget(dtype, k, a, b, alpha, c0 if add else None, diag)
    want = c0.double().clone()
    region = _mask(m, n, "full" if kind == "full" else kind)
    if ri is not None:
        blk = want[ri.long()[:, None], ci.long()[None, :]]
        base = blk if add else torch.zeros_like(blk)
        want[ri.long()[:, None], ci.long()[None, :]] = torch.where(region, base + prod, blk)
        region_full = torch.zeros((dm, dn), dtype=torch.bool, device="cuda")
        region_full[ri.long()[:, None], ci.long()[None, :]] = region
        region = region_full
    else:
        want = torch.where(region, (want if add else 0.0) + prod, want)
    a_in, b_in = _nan_outside(a, astruct), _nan_outside(b, bstruct)
    accum = F.ACCUM_ADD if add else F.ACCUM_REPLACE
    variant = int(extras.get("variant", 0))
    prob = gemm_row_problem(dtype, case[1:])
    strides = {"d": tuple(dst.stride()), "a": tuple(a_in.stride()), "b": tuple(b_in.stride())}
    _set_variant(F, variant)
    try:
        with Routes(F) as rt:
            if astruct != "rect" or bstruct != "rect" or kind.startswith("strict"):
                F.matmul_triangular(dst, "rect" if kind == "full" else kind, accum, a_in, astruct, b_in, bstruct, alpha)
            elif "neg_strides" in extras:
                # rows of A and columns of B reversed through hand-made views (torch has no negative strides)
                sa, sb = a.flip(0).clone(), b.flip(1).clone()  # stored reversed: the views read a, b
                isz = sa.element_size()
                va = F.MatRef(sa.data_ptr() + (m - 1) * sa.stride(0) * isz, m, k, -sa.stride(0), sa.stride(1))
                vb = F.MatRef(sb.data_ptr() + (n - 1) * sb.stride(1) * isz, k, n, sb.stride(0), -sb.stride(1))
                strides.update(a=(va.row_stride, va.col_stride), b=(vb.row_stride, vb.col_stride))
                al = (C.c_double if dtype == F64 else C.c_float)(alpha)
                getattr(F.lib(), f"libfaer_v0_23_matmul_{suffix(dtype)}")(F._mat(dst, F.MatMut), C.c_int(accum), va, vb, C.byref(al),
                                                                         F.PAR_SEQ)
            elif "huge_ld" in extras:
                # K-major rhs whose columns lie further apart than the 32-bit tile offsets of the pipelined loaders reach
                ld = (1 << 31) // (256 * a.element_size()) + 1000
                big = torch.zeros((n, ld), dtype=tdt, device="cuda")
                big[:, :k] = b.t()
                vb = big[:, :k].t()
                assert vb.stride() == (1, ld)
                strides["b"] = tuple(vb.stride())
                F.matmul(dst, accum, a_in, vb, alpha)
            else:
                dk = {"full": F.DST_FULL, "lower": F.DST_LOWER, "upper": F.DST_UPPER}[kind]
                F.gemm(dst, dk, accum, a_in, b_in, alpha, row_idx=ri, col_idx=ci, diag=diag)
    finally:
        _set_variant(F, 0)
    rt.assert_hit(route, *more)
    # what ran is what the dispatch plans for this call (faer_hip_debug_gemm_plan), no route more and none less; the level-2
    # kernels decide for themselves and count their own route only
    ran = {r for r, c in rt.hits.items() if c and r.startswith("Gemm")}
    if route in LEVEL2_ROUTES:
        assert ran == {route}, ran
    else:
        assert strides == {"d": (prob["drs"], prob["dcs"]), "a": (prob["ars"], prob["acs"]), "b": (prob["brs"], prob["bcs"])}, strides
        plan = F.debug_gemm_plan(**prob)
        assert isinstance(plan, dict), plan
        assert ran == {r for i, r in enumerate(ROUTES) if plan["routes"] >> i & 1}, (ran, plan)
    assert not any(rt.hits[r] for r in RETIRED)
    got = dst.double()
    exp = want.to(tdt).double()
    ok = (got == exp) | ~region
    if not bool(ok.all()):
        bad = (~ok).nonzero()[:8].tolist()
        pytest.fail(f"{int((~ok).sum())} entries differ from the exact product, first at {bad}: "
                    f"got {[got[i, j].item() for i, j in bad]} want {[exp[i, j].item() for i, j in bad]}")
    assert same_bits(dst[~region], c0[~region]), "entries outside the written part changed"
    if parent is not None:
        inside = torch.zeros(parent.shape, dtype=torch.bool, device="cuda")
        inside[3:3 + dm, 5:5 + dn] = True
        assert same_bits(parent[~inside], parent0[~inside]), "the parent changed outside the dst view"


# ------------------------------------------------------------------------------------------------ structured products
STRUCTS = ["rect", "lower", "upper", "strict_lower", "strict_upper", "unit_lower", "unit_upper"]


@pytest.mark.gpu
@pytest.mark.parametrize("cs", STRUCTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=suffix)
def test_triangular_products_are_exact(dtype, cs):
    """all 7^3 structure triples (matmul_triangular) at n = 1, 64, 65, 129, 700: the unstructured part of every operand is
    NaN (the diagonal too for unit / strict structures) and must not be read; dst outside its structure is unchanged bit for
    bit; inside, the exact product"""
    import torch

    F = init_gpu()
    tdt = tdtype(dtype)
    r = RANGE[np.dtype(dtype)]
    g = torch.Generator(device="cuda").manual_seed(STRUCTS.index(cs) + 100 * (dtype == F32))
    for ci_, (as_, bs_, n) in enumerate(itertools.product(STRUCTS, STRUCTS, [1, 64, 65, 129, 700])):
        add = ci_ % 2 == 0
        alpha = [1.0, -1.0, 2.0, -0.5][ci_ % 4]
        a, b = ints(g, (n, n), r, dtype), ints(g, (n, n), r, dtype)
        c0 = ints(g, (n, n), r, dtype)
        if not add:
            c0[_mask(n, n, cs)] = float("nan")  # Replace never reads the structured part
        a_in, b_in = _nan_outside(a, as_), _nan_outside(b, bs_)
        assert_exact_budget(dtype, n, a, b, alpha, c0)
        dst = c0.clone().t().contiguous().t()
        with Routes(F) as rt:
            F.matmul_triangular(dst, cs, F.ACCUM_ADD if add else F.ACCUM_REPLACE, a_in, as_, b_in, bs_, alpha)
        if as_ != "rect" or bs_ != "rect":
            rt.assert_hit("GemmExtra64")
        prod = alpha * (_dense(a.double(), as_) @ _dense(b.double(), bs_))
        reg = _mask(n, n, cs)
        want = ((c0.double() if add else 0.0) + prod).to(tdt)
        assert bool((dst[reg] == want[reg]).all()), (cs, as_, bs_, n, add, alpha)
        assert same_bits(dst[~reg], c0[~reg]), (cs, as_, bs_, n)


# ------------------------------------------------------------------------------------------------ TRSM
TRSM_N = [1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 1000, 2049]
TRSM_K = [1, 16, 17, 63, 64, 65, 300]
RHS_KINDS = ["F", "C", "strided", "reversed"]


def _trsm_cases():
    """every (n, k) pair of the grid once per dtype; side, unit, T order and rhs layout rotate so that each pair of those
    axes meets (and each of them meets every n), plus the wide solves that reach RW32 and the 128 non-pipelined tile"""
    out = []
    axes = list(itertools.product([False, True], [False, True], ["F", "C"], RHS_KINDS))  # 32 combinations
    for di, dt in enumerate(DTYPES):
        for idx, (n, k) in enumerate(itertools.product(TRSM_N, TRSM_K)):
            upper, unit, torder, rk = axes[(idx * 7 + di * 11) % len(axes)]
            out.append((dt, n, k, upper, unit, torder, rk))
        out += [(dt, 128, 20000, False, False, "F", "F"), (dt, 100, 20000, True, True, "C", "C"),
                (dt, 4096, 2100, True, False, "F", "F")]
    return out


TRSM_CASES = _trsm_cases()


def _trsm_routes(n, k):
    if n <= 64 and k < 64:
        return ("TrsmTiny",)
    if n <= 128:
        return ("TrsmLeafDirect32",) if k > 256 * 64 else ("TrsmLeafDirect16",)
    rs = ("TrsmRecursion", "TrsmLeafDirect32" if k > 256 * 64 else "TrsmLeafDirect16")
    return rs + (("GemmLegacy128",) if n >= 4096 and k >= 2049 else ())


def _trsm_id(c):
    dt, n, k, upper, unit, torder, rk = c
    return f"{suffix(dt)}-n{n}-k{k}-{'upper' if upper else 'lower'}-{'unit' if unit else 'nonunit'}-T{torder}-rhs{rk}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", TRSM_CASES, ids=_trsm_id)
def test_trsm_route_is_exact(case):
    """B = T X with integer X, T's off-diagonal in {-1, 0, 1} and its diagonal in {+-1, +-2, +-1/2, +-4} (the kernels multiply
    by the reciprocal of the diagonal, exact for these): every route returns X bit for bit.  The triangle the solve must not
    read holds NaN, and so does the diagonal of a unit solve."""
    import torch

    dtype, n, k, upper, unit, torder, rk = case
    F = init_gpu()
    tdt = tdtype(dtype)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(_trsm_id(case).encode()))
    r = 100 if dtype == F32 else 1 << 20
    off = torch.randint(-1, 2, (n, n), generator=g, device="cuda").double()
    pw = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0], dtype=torch.float64, device="cuda")
    d = torch.ones(n, dtype=torch.float64, device="cuda") if unit else pw[torch.randint(0, 8, (n,), generator=g, device="cuda")]
    t = (torch.triu(off, 1) if upper else torch.tril(off, -1)) + torch.diag(d)
    x = torch.randint(-r, r + 1, (n, k), generator=g, device="cuda").double()
    b = t @ x
    # budget: every partial sum of the substitution is a part of sum_j |t_ij| |x_j| <= (n - 1 + 4) r, in halves (diagonal 1/2)
    units, lim = exact_budget(dtype, n + 3, 1.0, float(r), frac=1)
    assert units < lim
    assert float(b.abs().max().item()) * 2 < 2.0 ** MANT[np.dtype(dtype)]
    tn = t.clone()
    tn[~_mask(n, n, ("strict_upper" if upper else "strict_lower") if unit else ("upper" if upper else "lower"))] = float("nan")
    td = tn.to(tdt)
    td = td.contiguous() if torder == "C" else td.t().contiguous().t()
    bt = b.to(tdt)
    parent = None
    isz = bt.element_size()
    if rk == "F":
        xv = bt.t().contiguous().t()
        view = F._mat(xv, F.MatMut)
    elif rk == "C":
        xv = bt.contiguous()
        view = F._mat(xv, F.MatMut)
    elif rk == "strided":
        parent = torch.full((2 * n + 1, 3 * k + 2), -3.25, dtype=tdt, device="cuda").t().contiguous().t()
        xv = parent[1::2, 2::3][:n, :k]
        xv.copy_(bt)
        view = F._mat(xv, F.MatMut)
    else:  # reversed rows inside a sentinel parent (a hand-made view with a negative row stride)
        parent = torch.full((n + 5, k + 7), -3.25, dtype=tdt, device="cuda").t().contiguous().t()
        parent[0, 0] = float("nan")
        xv = parent[2:2 + n, 3:3 + k]
        xv.copy_(bt.flip(0))
        view = F.MatMut(xv.data_ptr() + (n - 1) * xv.stride(0) * isz, n, k, -xv.stride(0), xv.stride(1))
    parent0 = parent.clone() if parent is not None else None
    name = {(False, False): "solve_triangular_lower_in_place", (True, False): "solve_triangular_upper_in_place",
            (False, True): "solve_unit_triangular_lower_in_place", (True, True): "solve_unit_triangular_upper_in_place"}[(upper, unit)]
    with Routes(F) as rt:
        getattr(F.lib(), f"libfaer_v0_23_{name}_{suffix(dtype)}")(F._mat(td), C.c_int(F.CONJ_NO), view, F.PAR_SEQ)
    rt.assert_hit(*_trsm_routes(n, k))
    got = xv.flip(0) if rk == "reversed" else xv
    want = x.to(tdt)
    if not torch.equal(got, want):
        ok = got == want
        bad = (~ok).nonzero()[:6].tolist()
        pytest.fail(f"{int((~ok).sum())} of {n * k} entries differ from X, first at {bad}: "
                    f"got {[got[i, j].item() for i, j in bad]} want {[want[i, j].item() for i, j in bad]}")
    if parent is not None:
        inside = torch.zeros(parent.shape, dtype=torch.bool, device="cuda")
        if rk == "strided":
            inside[1::2, 2::3][:n, :k] = True
        else:
            inside[2:2 + n, 3:3 + k] = True
        assert same_bits(parent[~inside], parent0[~inside]), "the parent changed outside the rhs view"


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=suffix)
def test_split_k_lower_dst_is_bitwise_reproducible(dtype):
    """split-K adds its slices in a fixed order (gemm.hip, gemm_dev): a direct call with a Lower dst on float data gives the
    same bits twice"""
    import torch

    F = init_gpu()
    tdt = tdtype(dtype)
    g = torch.Generator(device="cuda").manual_seed(3)
    m, k = 300, 8192
    a = torch.randn((k, m), dtype=tdt, device="cuda", generator=g).t()
    b = torch.randn((m, k), dtype=tdt, device="cuda", generator=g).t()
    c0 = torch.randn((m, m), dtype=tdt, device="cuda", generator=g).t().contiguous().t()
    outs = []
    for _ in range(2):
        c = c0.clone().t().contiguous().t()
        with Routes(F) as rt:
            F.gemm(c, F.DST_LOWER, F.ACCUM_ADD, a, b, -0.75)
        rt.assert_hit("GemmSplitK", "GemmTriEnum")
        outs.append(c)
    assert same_bits(outs[0], outs[1])
    lo = _mask(m, m, "lower")
    assert same_bits(outs[0][~lo], c0[~lo])


# ------------------------------------------------------------------------------------------------ CPU checks
def test_case_tables_name_every_route():
    """every FaerHipRoute is pinned by a row of the tables above in BOTH dtypes, or listed in DRIVER_ONLY with the test that
    reaches it (or why nothing can)"""
    assert ROUTES and "GemmSplitK" in ROUTES and "TrsmRecursion" in ROUTES
    named = {}
    for c in GEMM_CASES:
        for r in (c[1],) + tuple(c[10]):
            named.setdefault(r, set()).add(c[0])
    for c in TRSM_CASES:
        for r in _trsm_routes(c[1], c[2]):
            named.setdefault(r, set()).add(c[0])
    for r in ["GemmExtra64"]:  # test_triangular_products_are_exact
        named.setdefault(r, set()).update(DTYPES)
    unknown = (set(named) | set(DRIVER_ONLY)) - set(ROUTES)
    assert not unknown, unknown
    assert len(RETIRED) == 2 and not set(RETIRED) & (set(named) | set(DRIVER_ONLY))
    for r in ROUTES:
        if r in RETIRED:
            continue
        if r in DRIVER_ONLY:
            assert r not in named, f"{r} is pinned here: drop it from DRIVER_ONLY"
            why = DRIVER_ONLY[r]
            assert why.startswith("tests.") or "no driver" in why
            if why.startswith("tests."):
                mod, test = why.split("::")
                src = open(os.path.join(ROOT, *mod.split(".")) + ".py").read()
                assert f"def {test}(" in src, why
        else:
            assert named.get(r, set()) == set(DTYPES), f"route {r} is not pinned in both dtypes: {named.get(r)}"


def _exact_product(a, b, alpha, c0):
    """Python rational arithmetic: c0 + alpha * a b, no rounding anywhere"""
    m, k = len(a), len(a[0])
    n = len(b[0])
    al = Fraction(alpha)
    return [[Fraction(c0[i][j]) + al * sum(Fraction(a[i][p]) * Fraction(b[p][j]) for p in range(k)) for j in range(n)]
            for i in range(m)]


@pytest.mark.parametrize("dtype", DTYPES, ids=suffix)
def test_exactness_budget_against_python_integers(dtype):
    """cases the budget accepts are exact in `dtype` in any order: the fp64 reference cast to dtype, a float summation in
    dtype in two different orders and the rational result all agree; a case just outside is refused"""
    rng = np.random.default_rng(7)
    p = MANT[np.dtype(dtype)]
    for m, n, k, r, alpha in [(3, 4, 5, 15, -0.5), (2, 2, 64, 4095, 1.0), (5, 3, 17, 15, 2.0), (1, 1, 1000, 100, -1.0)]:
        a = rng.integers(-r, r + 1, (m, k)).astype(dtype)
        b = rng.integers(-r, r + 1, (k, n)).astype(dtype)
        c0 = rng.integers(-r, r + 1, (m, n)).astype(dtype)
        units, lim = exact_budget(dtype, k, float(np.abs(a).max()), float(np.abs(b).max()), alpha, float(np.abs(c0).max()),
                                  frac=frac_bits([alpha]))
        if units >= lim:
            with pytest.raises(AssertionError):
                assert_exact_budget(dtype, k, a, b, alpha, c0)
            continue
        assert_exact_budget(dtype, k, a, b, alpha, c0)
        exact = _exact_product(a.tolist(), b.tolist(), alpha, c0.tolist())
        ref = (c0.astype(np.float64) + alpha * (a.astype(np.float64) @ b.astype(np.float64))).astype(dtype)
        fwd = c0.copy()
        bwd = np.zeros_like(c0)
        for q in range(k):  # dtype arithmetic, two summation orders
            fwd = (fwd + dtype(alpha) * np.outer(a[:, q], b[q, :]).astype(dtype)).astype(dtype)
            bwd = (bwd + np.outer(a[:, k - 1 - q], b[k - 1 - q, :]).astype(dtype)).astype(dtype)
        bwd = (c0 + dtype(alpha) * bwd).astype(dtype)
        for i in range(m):
            for j in range(n):
                assert Fraction(float(ref[i, j])) == exact[i][j]
                assert fwd[i, j] == ref[i, j] and bwd[i, j] == ref[i, j]
    # just outside the range: refused before any call
    big = float(2 ** (p // 2 + 1))
    with pytest.raises(AssertionError):
        assert_exact_budget(dtype, 4, np.full((2, 4), big), np.full((4, 2), big))
    # the half bit of alpha = -0.5 counts
    edge = float(2 ** ((p - 2) // 2))
    assert_exact_budget(dtype, 1, np.full((1, 1), edge), np.full((1, 1), edge), 1.0)
    with pytest.raises(AssertionError):
        assert_exact_budget(dtype, 4, np.full((1, 4), edge), np.full((4, 1), edge), -0.5)
