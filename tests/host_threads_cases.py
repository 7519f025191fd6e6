"""The case table and the schedules of tests/test_gpu_host_threads.py (independent library calls from concurrent host threads).
Plain data and integer logic: importable without a GPU (tests/test_host_threads_cases.py checks it there).

A case name is "<what>:<type>".  For the small table <what> is an entry of test_gpu_stream_order.SMALL (inputs and calls: make / call
of that module); the other cases restate the shapes of the tests named at each of them (host_threads_worker.py builds them).

Equality classes -- how a result computed beside other threads' calls is compared with the same call made alone:
  bitwise  every output bit for bit, indices / counts / status exactly (gpu_util.same_result);
  pivots   identical pivots and counts, factors at the bound of test_gpu_stream_order.test_plu (the recursion of LU 1000 x 1000, which
           no test asserts to repeat itself bit for bit);
  bounded  as `pivots`, at the parity bound of the case's family: only for a cooperative case whose panel kernel was seen to give up its
           exchange under contention and to finish on the non-cooperative path.  BOUNDED_ALLOWED is the cap; BOUNDED is what sits
           there now, each with its reason."""
from test_gpu_stream_order import SMALL

THREAD_COUNTS = (2, 3)

# ---- the small table: one blocked shape per family (the distributed drivers in fp64 only, like test_gpu_stream_order.test_small)
SMALL_F64 = [f"{f}:f64" for f in SMALL]
SMALL_F32 = [f"{f}:f32" for f in SMALL if not f.startswith("dist")]

# ---- cases that own internal streams or cooperative panel kernels
LLT_LA = "llt_la_3077:f64"          # test_llt_lookahead 3077-tail-1024 (FAER_HIP_LLT_LA_MIN=2048, FAER_HIP_LLT_TAIL=1024)
LLT_STEP_KINDS_CASE = "llt_step_kinds_5197:f64"  # test_llt_lookahead 5197-step-kinds-f64 (LLT_STEP_KINDS, tail 0)
LU_LA = "lu_la_3072:f64"            # test_plu_lookahead under faer_hip_debug_lu_plan(512, 1536, 2048)
LU_COOP = "lu_600x5:f64"            # test_plu (600, 5): the cooperative leaf
LU_REC = "lu_1000x1000:f64"         # test_plu (1000, 1000): the recursion
QR_ONE_PASS_F32 = "qr_20000x64_bs64:f32"   # test_qr: the one-pass tall path
QR_ONE_PASS_F64 = "qr_16500x17_bs1:f64"
QR_MIXED = "qr_2100x800_bs192:f64"  # the classic driver whose recursion hands panels to the one-pass panel kernel
QR_CLASSIC = "qr_512x200_bs32:f64"
# ---- the newer families, each with the inputs and call sequence of its own module's caller-stream test
CLU_700 = "clu_700:c64"             # test_gpu_complex_lu.test_factor_and_solve_on_a_caller_stream
CLU_STEP = "clu_5000x40:c64"        # the column-step case of test_gpu_complex_lu.test_poisoned_pool
CMATMUL = "cmatmul_300x200x1000:c64"  # test_gpu_complex_matmul.test_matmul_on_a_caller_stream
CTRSM = "ctrsm_poisoned_pool_sizes:c32"  # test_gpu_complex_trsm.test_poisoned_pool: host operands, c64 product 129 x 127 x 130, c32 solve 129 x 33
CHOL_UPDATE = ["chol_update:f64", "chol_update:f32"]  # test_gpu_chol_update.test_stream_order
EVD_GENERAL = ["evd_general:f64", "evd_general:f32"]  # test_gpu_evd_general.test_non_blocking_caller_stream (both sizes)
GEVD = ["gevd:f64", "gevd:f32"]                       # test_gpu_gevd.test_non_blocking_caller_stream (both sizes)

# every unordered pair of these meets in phase C of the look-ahead group, and each meets a level-2 family and the wide product
CONTENDED = [LU_LA, LU_COOP, QR_ONE_PASS_F64, QR_MIXED, CLU_STEP, LLT_LA]
LEVEL2 = ["tridiag:f64", "fplu:f64"]
PRODUCT = "matmul_wide:f64"

# (same-family cases sit len // 2 apart, so that the two of them meet in the offset walk of T = 2: each reads its own counters)
NEWER = [CLU_700, CMATMUL, CHOL_UPDATE[0], EVD_GENERAL[0], GEVD[0], CLU_STEP, CTRSM, CHOL_UPDATE[1], EVD_GENERAL[1], GEVD[1]]

# group -> the cases of phase B (the same case on every thread); R runs each
GROUPS = {
    "small-f64": SMALL_F64,
    "small-f32": SMALL_F32,
    "look-ahead": [LLT_LA, LU_LA, LU_COOP, LU_REC],
    "llt-step-kinds": [LLT_STEP_KINDS_CASE],
    "qr": [QR_ONE_PASS_F32, QR_ONE_PASS_F64, QR_MIXED, QR_CLASSIC],
    "newer-families": NEWER,
    "default-queues": SMALL_F64,  # the last pass: T = 2, the inherited GPU_MAX_HW_QUEUES
}
RUNS = {"small-f64": 3, "small-f32": 3, "default-queues": 3, "look-ahead": 2, "llt-step-kinds": 2, "qr": 2, "newer-families": 2}
# environment of a group's child, set before the library loads
ENV = {
    "look-ahead": {"FAER_HIP_LLT_LA_MIN": "2048", "FAER_HIP_LLT_TAIL": "1024"},
    "llt-step-kinds": {"FAER_HIP_LLT_LA_MIN": "2048", "FAER_HIP_LLT_TAIL": "0"},  # + test_gpu_factor.LLT_STEP_KINDS, added by the test
}
# the groups that are not tables of cases
STATUS_ROUNDS = 3
LIFETIME_GENERATIONS = 8
LIFETIME_CASES = ["llt_rebuild:f64", "matmul_split_k:f64"]

ALL_CASES = sorted({c for g in GROUPS.values() for c in g} | set(CONTENDED) | set(LEVEL2) | {PRODUCT})

# ---- equality classes
BOUNDED_ALLOWED = {LU_COOP, LU_LA, QR_ONE_PASS_F32, QR_ONE_PASS_F64, QR_MIXED, CLU_STEP}
BOUNDED = {}  # case -> reason (the captured fallback message and the path that took it); empty: nothing had to move
PIVOTS = {LU_REC}


def equality_class(case):
    classes = [name for name, members in (("bounded", BOUNDED), ("pivots", PIVOTS)) if case in members]
    assert len(classes) <= 1, (case, classes)
    return classes[0] if classes else "bitwise"


# ---- phase C: different cases at once
def phase_c_table(group):
    """the cases phase C of a group walks.  The look-ahead group's is the cross-family one: the cases that own internal streams or
    cooperative kernels (its own, the QR group's and the complex LU's column steps) with a level-2 family and the wide product"""
    if group == "look-ahead":
        return CONTENDED + LEVEL2 + [PRODUCT, LU_REC]
    return list(GROUPS[group])


def required_pairs(group):
    if group != "look-ahead":
        return set()
    pairs = {frozenset((a, b)) for i, a in enumerate(CONTENDED) for b in CONTENDED[i + 1:]}
    for i, c in enumerate(CONTENDED):
        pairs.add(frozenset((c, LEVEL2[i % len(LEVEL2)])))
        pairs.add(frozenset((c, PRODUCT)))
    return pairs


def _pairs_of(step):
    return {frozenset((a, b)) for i, a in enumerate(step) for b in step[i + 1:]}


def _combinations(items, k):
    if k == 0:
        yield ()
        return
    for i, x in enumerate(items):
        for rest in _combinations(items[i + 1:], k - 1):
            yield (x,) + rest


def schedule(group, threads):
    """phase C as a list of steps; step[t] is the case thread t runs, all cases of a step distinct.  A plain group: thread t walks the
    table from offset t * (len // threads), so every thread runs every case once.  The look-ahead group: steps chosen greedily (always
    the one that covers most of the pairs still missing, first in table order among equals) until every required pair has met, then the
    cases not yet seen beside the first ones of the table; the places of a step rotate so that a case is not always thread 0's."""
    table = phase_c_table(group)
    n = len(table)
    if n < threads:
        return []
    need = required_pairs(group)
    if not need:
        off = n // threads
        return [tuple(table[(s + t * off) % n] for t in range(threads)) for s in range(n)]
    steps = []
    candidates = list(_combinations(table, threads))
    while need:
        best = max(candidates, key=lambda c: len(_pairs_of(c) & need))  # (max keeps the first of equals)
        assert _pairs_of(best) & need
        need -= _pairs_of(best)
        steps.append(best)
    seen = {c for s in steps for c in s}
    for c in table:
        if c not in seen:
            steps.append((c,) + tuple(x for x in table if x != c)[:threads - 1])
    return [s[i % threads:] + s[:i % threads] for i, s in enumerate(steps)]
