"""The dense GEMM dispatch as data (csrc/gemm.hip gemm_orient + gemm_plan, through faer_hip_debug_gemm_plan): no GPU needed.

1. Every dense row of the exact-integer table of test_gpu_level3_exact.py plans the routes the row names, for the shapes and
   strides the GPU test builds.
2. Over a grid of shapes, layouts and options the plan equals the one-function dispatch it replaced, written out below line by
   line as it stood (old_dispatch): every field, and the same message where the product is refused."""
import ctypes as C
import itertools

from gpu_util import ROUTES, fa
from test_gpu_level3_exact import DTYPES, GEMM_ROWS, gemm_row_problem

LEVEL2 = {"GemmZeroK", "GemmRank1", "GemmGemv", "GemmSkinny"}
FULL, LOWER, UPPER = 0, 1, 2
R = {name: i for i, name in enumerate(ROUTES)}


def route_set(mask):
    return {r for i, r in enumerate(ROUTES) if mask >> i & 1}


def test_rows_of_the_exact_table_plan_their_routes():
    F = fa()
    assert F.GEMM_TILES == tuple(r[4:] for r in ROUTES[5:9] + ROUTES[11:13])  # tile kinds are named like their routes
    dense = [row for row in GEMM_ROWS if row[0] not in LEVEL2]
    assert len(dense) == len(GEMM_ROWS) - 8
    for dtype, row in itertools.product(DTYPES, dense):
        plan = F.debug_gemm_plan(**gemm_row_problem(dtype, row))
        assert isinstance(plan, dict), (row, plan)
        want = {row[0]} | set(row[9])
        got = route_set(plan["routes"])
        assert want <= got, (row, got)
        assert "Gemm" + F.GEMM_TILES[plan["tile"]] in got
        # the fields behind the "further routes"
        assert ("GemmTransposed" in got) == bool(plan["transposed"]) and ("GemmTriEnum" in got) == bool(plan["tri_enum"])
        assert ("GemmSplitK" in got) == (plan["splits"] > 1)
        assert {f"GemmFastIo{plan['fast_io']}"} - {"GemmFastIo0"} == {r for r in got if r.startswith("GemmFastIo")}


# ------------------------------------------------------------------------------------------------ the dispatch it replaced
def tri_tiles(rows, wide):
    if not wide:
        return rows * (rows + 1) // 2
    p = rows // 2
    return (p + 1) * (p + 1) if rows & 1 else p * (p + 1)


def old_dispatch(m, n, k, ts, kind, add, alpha_sign, drs, dcs, ars, acs, brs, bcs, indexed, diag, a_struct, b_struct, k_trim, tri_skip,
                 stair_nb, stair_gap, stair_row0, prefer_big_tiles, variant):
    """gemm_dev from its transposition to its launch as it stood before gemm_plan, statement by statement: `shape`, `big`, `wide`,
    `legacy` and `extra_path` assigned in its order, then the route chain and the launch chain.  Returns the plan's fields in
    the order of faer_rs_amd.GEMM_PLAN_FIELDS, or the message of the FH_CHECK that fires."""
    hits = set()
    transpose = kind == UPPER or (kind == FULL and abs(dcs) == 1 and abs(drs) != 1 and not indexed)
    if transpose:
        hits.add("GemmTransposed")
        drs, dcs = dcs, drs
        ars, acs, brs, bcs = bcs, brs, acs, ars  # A <- B^T, B <- A^T
        if k_trim:
            k_trim = 3 - k_trim
        m, n = n, m
        tr = [0, 2, 1, 4, 3, 6, 5]
        a_struct, b_struct = tr[b_struct], tr[a_struct]
        if kind == UPPER:
            kind = LOWER
    lower = kind == LOWER
    extra_path = bool(diag or a_struct or b_struct)
    if k_trim or tri_skip or stair_nb:
        if not (not extra_path and not indexed and variant < 10):
            return "gemm: k_trim / tri_skip / stair_nb need the plain dense kernel"
    if stair_nb:
        if not (lower and not transpose and stair_nb > 0 and stair_gap >= 0 and stair_row0 >= 0):
            return "gemm: stair_nb needs a lower, untransposed dst"
    akm = abs(acs) == 1 and abs(ars) != 1
    bkm = abs(brs) == 1 and abs(bcs) != 1
    tiles128 = ((m + 127) // 128) * ((n + 127) // 128) // (2 if lower else 1)
    big = tiles128 >= 256
    if variant in (1, 11, 3):
        big = True
    if variant in (2, 12):
        big = False
    if (variant == 6 or (variant == 0 and prefer_big_tiles)) and not big and kind == FULL and k >= 2048 and (
            (m >= 128 and n >= 1024) or (n >= 128 and m >= 1024)):
        big = True
    legacy = variant >= 10
    a_ok = ars >= 0 and acs >= 0 and (akm or ((m - 1) * ars + 32 * acs) * ts < (1 << 31))
    b_ok = brs >= 0 and bcs >= 0 and ((bcs >= 16 and (16 * brs + 256 * bcs) * ts < (1 << 31)) if bkm
                                      else ((n - 1) * bcs + 32 * brs) * ts < (1 << 31))
    if not (a_ok and b_ok) and not legacy:
        if tri_skip and not k_trim and not stair_nb:
            if not (lower and m == n and tri_skip < m):
                return "gemm: tri_skip needs a square lower dst"
            hits.add("GemmTriSkipSplit")
            return [int(transpose), 0, 1, int(akm), int(bkm)] + 10 * [0] + [sum(1 << R[h] for h in hits)]
        if not (not k_trim and not tri_skip and not stair_nb):
            return "gemm: operand strides out of range for this product"
        legacy = True
    plain = not diag and not a_struct and not b_struct and not indexed
    wide_ok = plain and ((not k_trim) if kind == FULL else (m == n))
    tiles_wide = ((m + 127) // 128) * ((n + 255) // 256)
    wide_auto = kind == FULL and k >= 2048 and tiles_wide >= 512
    wide = wide_ok and big and variant != 5 and not legacy and (variant == 3 or (variant == 0 and wide_auto))
    bm = bn = 128 if big else 64
    shape = 0 if big else 1
    if extra_path:
        bm = bn = 64
        shape = 1
    if wide:
        bm, bn, shape = 128, 256, 5
    ntm = (m + bm - 1) // bm
    ntn = (n + bn - 1) // bn
    tri_enum = int(lower and m == n and not stair_nb)
    tri_off = 0
    if tri_skip:
        if not (tri_enum and tri_skip % bm == 0 and tri_skip < m):
            return "gemm: tri_skip needs a square lower dst and a tile-aligned skip"
        tri_off = tri_tiles(tri_skip // bm, bn == 2 * bm)
    tiles = tri_tiles(ntm, bn == 2 * bm) - tri_off if tri_enum else ntm * ntn
    splits = 1
    mink, chunk = (1024, 256) if kind == FULL else (4096, 1024)
    if tiles < 256 and k >= mink and not indexed and not k_trim and not stair_nb:
        splits = (512 + tiles - 1) // tiles
        splits = min(splits, k // chunk, 1024)
        splits = max(splits, 1)
    kps = (k + splits - 1) // splits
    kps = (kps + 15) // 16 * 16
    splits = (k + kps - 1) // kps
    fast_io = 0
    if plain and not legacy and splits == 1 and drs == 1 and 0 < dcs < (1 << 21) and not stair_nb:
        if not add:
            fast_io = 1
        elif alpha_sign == 1:
            fast_io = 2
        elif alpha_sign == -1:
            fast_io = 3
    prof_class = 0 if not extra_path and not legacy and shape in (0, 5) else -1
    if tri_enum:
        hits.add("GemmTriEnum")
    if splits > 1:
        hits.add("GemmSplitK")
    if fast_io:
        hits.add(f"GemmFastIo{fast_io}")
    # the route chain
    hits.add("GemmExtra64" if extra_path else "GemmPipeWide" if shape == 5
             else ("GemmLegacy128" if shape == 0 else "GemmLegacy64") if legacy
             else "GemmPipe128" if shape == 0 else "GemmPipe64")
    # the launch chain: launch_cfg<64, 64, EXTRA> / launch_cfg_p<128, 256> / launch_cfg<128, 128> / <64, 64> / launch_cfg_p<128, 128> / <64, 64>
    tile = 0 if extra_path else 3 if shape == 5 else (5 if shape == 0 else 4) if legacy else 2 if shape == 0 else 1
    return [int(transpose), tile, 0, int(akm), int(bkm), bm, bn, ntm, ntn, tri_enum, tri_off, splits, kps, fast_io, prof_class,
            sum(1 << R[h] for h in hits)]


SIZES = [1, 63, 64, 65, 128, 129, 300, 2047, 2048, 2944, 4096]
# (m, n): every square, and every size once as m and once as n next to sizes from the other end of the list.  The full 11 x 11
# product is 8.7 million plans, minutes of Python for the line-by-line mirror; no other axis is thinned.
MN = [(s, s) for s in SIZES] + [(s, SIZES[(i + 5) % 11]) for i, s in enumerate(SIZES)] + [(4096, 2048), (2048, 4096), (128, 2048), (2944, 129)]
KS = [15, 16, 1023, 1024, 2048, 4099]
VARIANTS = [0, 1, 2, 3, 5, 6, 11, 12]
ACCUM = [(1, 1), (1, -1), (1, 0), (0, 1)]  # Add with alpha 1, -1, -0.5; Replace
EXTRAS = [{}, {"diag": 1}, {"a_struct": 1}, {"indexed": 1}, {"k_trim": 1}, {"k_trim": 2}, {"tri_skip": 128},
          {"stair_nb": 128, "stair_gap": 256, "stair_row0": 0}, {"prefer_big_tiles": 1}]


def layouts(m, n, k, ts):
    """(dst, lhs, rhs) strides: column major, row major, K major; then one view each the buffer-addressed loaders cannot take"""
    col = (1, m, 1, m, 1, k)
    huge = (1 << 31) // (256 * ts) + 1000
    return [col, (n, 1, k, 1, n, 1), (1, m, k, 1, 1, k),
            (1, m, -1, m, 1, -k),  # rows of lhs and columns of rhs reversed
            (1, m, 1, m, 1, 0),  # broadcast rhs column
            (1, m, 1, m, 1, 8),  # overlapping rhs columns
            (1, m, 1, m, 1, huge)]  # leading dimension beyond the 32-bit tile offsets


def test_plan_equals_the_one_function_dispatch_over_a_grid():
    F = fa()
    lib = F.lib()
    names = F.GEMM_PLAN_INPUTS
    inp = (C.c_longlong * len(names))()
    out = (C.c_int * len(F.GEMM_PLAN_FIELDS))()
    why = C.c_char_p()
    pwhy = C.byref(why)
    count = refused = 0
    seen_tiles, seen_msgs = set(), set()
    for (m, n), k, ts, kind in itertools.product(MN, KS, (8, 4), (FULL, LOWER, UPPER)):
        for lay, (add, sign), variant, ex in itertools.product(layouts(m, n, k, ts), ACCUM, VARIANTS, EXTRAS):
            if "tri_skip" in ex and not (kind == LOWER and m == n):
                continue
            q = dict(m=m, n=n, k=k, elem_bytes=ts, kind=kind, add=add, alpha_sign=sign, drs=lay[0], dcs=lay[1], ars=lay[2], acs=lay[3],
                     brs=lay[4], bcs=lay[5], variant=variant, **ex)
            inp[:] = args = [q.get(f, 0) for f in names]
            rc = lib.faer_hip_debug_gemm_plan(inp, out, pwhy)
            want = old_dispatch(*args)
            got = list(out) if rc == 0 else why.value.decode()
            assert rc in (0, 1) and got == want, (q, dict(zip(F.GEMM_PLAN_FIELDS, got)) if rc == 0 else got, want)
            count += 1
            if rc:
                refused += 1
                seen_msgs.add(got)
            else:
                seen_tiles.add(got[1] if not got[2] else "split")
    # the grid reaches every tile kind, the split and every refusal
    assert seen_tiles == {0, 1, 2, 3, 4, 5, "split"} and len(seen_msgs) == 5, (seen_tiles, seen_msgs)
    assert count > 1500000 and 0 < refused < count


def test_not_a_dense_product():
    F = fa()
    assert F.debug_gemm_plan(m=0, n=4, k=4, elem_bytes=8) is None and F.debug_gemm_plan(m=4, n=4, k=0, elem_bytes=8) is None
    assert F.debug_gemm_plan(m=4, n=4, k=4, elem_bytes=2) is None and F.debug_gemm_plan(m=1 << 31, n=4, k=4, elem_bytes=8) is None
