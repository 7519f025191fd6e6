"""The child process of tests/test_gpu_host_threads.py: independent library calls from T concurrent host threads of ONE process.

    python host_threads_worker.py GROUP T OUT.json

GROUP is a key of host_threads_cases.GROUPS, or "status" or "lifetime".  Every worker thread binds device 0, creates a non-blocking
torch stream of its own, enters it, hands it to the library (use_torch_stream) and waits for that stream only; ctypes releases the
GIL during the library's calls.  Inputs, calls and comparisons are those of tests/test_gpu_stream_order.py and of the newer families'
own caller-stream tests, imported from there.  Nothing raises past a thread: every mismatch becomes a line of `failures` in OUT.json
and the threads go on to the next barrier, so one wrong result cannot leave the others waiting."""
import ctypes as C
import json
import os
import sys
import threading
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import host_threads_cases as hc  # noqa: E402
from gpu_util import EPS, Routes, _fresh, fa, same_result, spd  # noqa: E402
from test_gpu_stream_order import GOOD, call, close_result, llt_fn, lu_fn, make, randn_dev, rnd, spd_dev  # noqa: E402

DTYPE = {"f64": np.float64, "f32": np.float32, "c64": np.complex128, "c32": np.complex64}
BARRIER_TIMEOUT = 120.0  # seconds; a thread that never arrives breaks the barrier for the others instead of hanging the child
LU_LA_PLAN = (512, 1536, 2048)


class Case:
    """inputs: {name: numpy array or device tensor}, never written; fn(bufs) -> {name: tensor / array / host value}; diag: the
    per-thread counters the case is about; host: the operands stay host memory (staged by the library)"""

    def __init__(self, inputs, fn, diag=(), host=False, check=None):
        self.inputs, self.fn, self.diag, self.host, self.check = inputs, fn, tuple(diag), host, check
        self.last_span = {}  # thread id -> (start, end) of its last run, host clock: from the call to the end of its stream's work


# ------------------------------------------------------------------------------------------ the cases
def build_case(F, name):
    import torch

    what, tname = name.split(":")
    dtype = DTYPE[tname]
    if f"{what}:f64" in hc.SMALL_F64:
        diag = {"lblt": ("lblt_last",), "piv_llt": ("piv_llt_last",), "qr_rebuild": ("qr_cols",)}.get(what, ())
        return Case(make(what, GOOD + len(what), dtype), lambda b: call(F, what, b), diag, check=lambda e: e.get("tag", 0) == 0)
    if name in (hc.LLT_LA, hc.LLT_STEP_KINDS_CASE):
        n = 3077 if name == hc.LLT_LA else 5197
        return Case({"a": spd_dev(n, GOOD + n, dtype)}, llt_fn(F), check=lambda e: e["count"] == 0)
    if name == hc.LU_LA:
        return Case({"a": randn_dev(3072, 3072, GOOD + 3072, dtype)}, lu_fn(F))
    if name in (hc.LU_COOP, hc.LU_REC):
        m, n = (600, 5) if name == hc.LU_COOP else (1000, 1000)
        return Case({"a": rnd(np.random.default_rng(GOOD + m), m, n, dtype)}, lu_fn(F))
    if what.startswith("qr_"):
        shape, bs = what[3:].split("_bs")
        m, n = (int(v) for v in shape.split("x"))
        bs, size = int(bs), min(m, n)

        def qr(b):
            rank = F.qr_factor_in_place(b["a"], b["h"])
            return {"rank": rank, "cols": F.lib().faer_hip_debug_qr_one_pass_columns(), "qr": b["a"], "h": b["h"]}

        cols = {hc.QR_ONE_PASS_F32: n, hc.QR_ONE_PASS_F64: n, hc.QR_MIXED: -1, hc.QR_CLASSIC: -1}[name]
        return Case({"a": rnd(np.random.default_rng(GOOD + m + n), m, n, dtype), "h": np.zeros((bs, size), dtype=dtype)}, qr, ("qr_cols",),
                    check=lambda e: e["rank"] == size and e["cols"] == cols)
    if name in (hc.CLU_700, hc.CLU_STEP):
        import complex_lu_ref as ref

        m, n = (700, 700) if name == hc.CLU_700 else (5000, 40)
        inputs = {"a": ref.gaussian(m, n, dtype, 7 + m + 3 * n)}  # (the matrix of test_gpu_complex_lu.reference(m, n, dtype))
        if m == n:
            inputs["b"] = ref.gaussian(n, 3, dtype, 1001)

        def clu(b):
            perm, perm_inv, nt = F.partial_piv_lu_factor_in_place(b["a"])
            out = {"lu": b["a"], "perm": perm, "perm_inv": perm_inv, "nt": nt}
            if "b" in b:
                F.partial_piv_lu_solve_in_place(b["a"], perm, perm_inv, b["b"], transpose=True, conj=True)
                out["x"] = b["b"]
            return out

        return Case(inputs, clu, ("clu_last",), check=lambda e: sorted(e["perm"].tolist()) == list(range(m)))
    if name == hc.CMATMUL:
        import complex_cases as cc

        m, n, k = 300, 200, 1000
        a, b, _, _, _ = cc.matmul_case(m, n, k, dtype)

        def cmm(bufs):
            F.matmul(bufs["c"], F.ACCUM_REPLACE, bufs["a"], bufs["b"], 2 - 1j)
            return {"c": bufs["c"]}

        return Case({"a": np.array(a), "b": np.array(b), "c": np.full((m, n), np.nan + 1j * np.nan, order="F")}, cmm)
    if name == hc.CTRSM:
        import complex_cases as cc

        m, n, k = 129, 127, 130
        a, b, _, _, _ = cc.matmul_case(m, n, k, np.complex128)
        t, rhs = cc.trsm_case(129, 33, np.complex64, "upper", False)

        def ctrsm(bufs):
            F.matmul(bufs["c"], F.ACCUM_REPLACE, bufs["a"], bufs["b"], 2 - 1j)
            F.solve_upper_triangular_in_place(bufs["tp"], bufs["x"], conj=True)
            return {"c": bufs["c"], "x": bufs["x"]}

        return Case({"a": np.array(a), "b": np.array(b), "c": np.full((m, n), np.nan + 1j * np.nan, order="F"), "tp": cc.tri_poisoned(t, "upper", False),
                     "x": np.array(rhs)}, ctrsm, host=True, check=lambda e: np.isfinite(e["c"]).all() and np.isfinite(e["x"]).all())
    if what == "chol_update":
        import test_gpu_chol_update as cu

        nb, rc = cu.shape(dtype)
        f, w, alpha = cu.ref_update(2 * nb + 1, rc + 1, dtype, False, False)[:3]

        def upd(b):
            return {"index": F.llt_rank_r_update_clobber(b["l"], b["w"], b["alpha"], raise_on_error=False), "l": b["l"]}

        return Case({"l": f, "w": w, "alpha": alpha}, upd, ("chol_update_last",), check=lambda e: e["index"] is None)
    if what in ("evd_general", "gevd"):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        if what == "evd_general":
            import evd_cases as ec
            import test_gpu_evd_general as eg

            sizes = eg.family_sizes(dtype)
            inputs = {f"a{n}": np.asfortranarray(ec.make("normal01", n, dtype)[0]) for n in sizes}
        else:
            import gevd_cases as gc
            import test_gpu_gevd as gg

            sizes = gg.family_sizes(dtype)
            inputs = {}
            for n in sizes:
                ga, gb = gc.generate("random", n, dtype)
                inputs[f"a{n}"], inputs[f"b{n}"] = np.asfortranarray(ga), np.asfortranarray(gb)

        def eig(b):
            out = {}
            for n in sizes:
                vecs = [torch.full((n,), -7.5, dtype=tdt, device="cuda") for _ in range(2 if what == "evd_general" else 3)]
                ul, ur = (torch.full((n, n), -7.5, dtype=tdt, device="cuda").t() for _ in range(2))
                if what == "evd_general":
                    out[f"tag{n}"] = F.evd(b[f"a{n}"], vecs[0], vecs[1], ul, ur)
                else:
                    out[f"tag{n}"] = F.generalized_evd(b[f"a{n}"], b[f"b{n}"], vecs[0], vecs[1], vecs[2], ul, ur)
                out.update({f"v{i}_{n}": v for i, v in enumerate(vecs)})
                out[f"ul{n}"], out[f"ur{n}"] = ul, ur
            return out

        ok = F.EVD_OK if what == "evd_general" else F.GEVD_OK
        return Case(inputs, eig, ("evd_counts" if what == "evd_general" else "gevd_counts",), check=lambda e: all(e[f"tag{n}"] == ok for n in sizes))
    raise ValueError(name)


DIAG = {
    "clu_last": lambda F: F.debug_clu_last(),
    "lblt_last": lambda F: list(F.debug_lblt_last()),
    "piv_llt_last": lambda F: list(F.debug_piv_llt_last()),
    "chol_update_last": lambda F: list(F.debug_chol_update_last()),
    "evd_counts": lambda F: F.debug_evd_last_counts(),
    "gevd_counts": lambda F: F.debug_gevd_last_counts(),
    "qr_cols": lambda F: int(F.lib().faer_hip_debug_qr_one_pass_columns()),
}


def to_host(out):
    """host values; complex arrays as their real components, so that same_result compares their bits"""
    import torch

    res = {}
    for k, v in out.items():
        if torch.is_tensor(v):
            v = v.detach().cpu().numpy()
        if isinstance(v, np.ndarray) and v.dtype.kind == "c":
            v = np.ascontiguousarray(v).view(np.float64 if v.dtype == np.complex128 else np.float32)
        res[k] = v
    return res


def prepare(case):
    """fresh copies of the inputs for one run (device copies on the calling thread's current stream)"""
    return {k: np.array(v, order="F") for k, v in case.inputs.items()} if case.host else _fresh(case.inputs)


def run_case(F, case, stream, bufs=None):
    """one run on the calling thread's stream: (host outputs, diagnostics read right after the call)"""
    bufs = prepare(case) if bufs is None else bufs
    with Routes(F) as r:
        t0 = time.perf_counter()
        out = case.fn(bufs)
        stream.synchronize()  # that stream only
        case.last_span[threading.get_ident()] = (t0, time.perf_counter())
    diag = {k: DIAG[k](F) for k in case.diag}
    diag["routes"] = {k: int(v) for k, v in r.hits.items() if v}
    return to_host(out), diag


# ------------------------------------------------------------------------------------------ comparison
_BOUNDS = {}


def parity_bound(name, case, expected):
    """{output: absolute entrywise bound} of the family's own parity test, for the classes `pivots` and `bounded`; from the inputs
    and the baseline alone, computed once per case"""
    if name not in _BOUNDS:
        _BOUNDS[name] = _parity_bound(name, case, expected)
    return _BOUNDS[name]


def _parity_bound(name, case, expected):
    a = case.inputs["a"]
    a = a.cpu().numpy() if not isinstance(a, np.ndarray) else a
    m, n = a.shape
    what, tname = name.split(":")
    eps = EPS[np.dtype(np.float64 if tname in ("f64", "c64") else np.float32)]
    if what.startswith("qr_"):  # test_qr_classic_path_one_pass_panels_vs_oracle, as test_gpu_stream_order.test_qr restates it
        tol = 64 * max(m, n) * eps * max(1.0, np.abs(a).max())
        return {"qr": 8 * tol, "h": 8 * tol * max(1.0, np.abs(expected["h"]).max())}
    size = min(m, n)
    kappa = np.linalg.cond(a[expected["perm"].astype(np.int64)][:size, :size])
    factor = 12 if what.startswith("clu") else 4  # test_gpu_complex_lu.check_factor / test_plu_vs_oracle
    return {"lu": factor * max(m, n) * eps * kappa * max(1.0, np.abs(expected["lu"]).max())}


def compare(name, case, base, got, diag, what):
    """None, or what differs between a thread's run (got, diag) and the baseline of the case"""
    expected, diag0 = base
    cls = hc.equality_class(name)
    notes = []
    try:
        if cls == "bitwise":
            same_result(expected, got, what)
        else:
            close_result(expected, got, parity_bound(name, case, expected), what)
    except AssertionError as ex:
        notes.append(f"{cls}: {ex}")
        if cls == "bitwise" and name in hc.BOUNDED_ALLOWED:  # what the bounded class would have said: the finding's other half
            try:
                close_result(expected, got, parity_bound(name, case, expected), what)
                notes.append("(identical indices and counts, inside the family's parity bound)")
            except AssertionError as ex2:
                notes.append(f"(bounded class as well: {ex2})")
    if diag != diag0:
        notes.append(f"diagnostics {diag} != the baseline's {diag0}")
    return f"{what}: " + "; ".join(notes) if notes else None


# ------------------------------------------------------------------------------------------ the groups of cases
class Run:
    def __init__(self, F, threads):
        self.F, self.threads = F, threads
        self.failures, self.lock = [], threading.Lock()
        self.info = {}
        self.barrier = threading.Barrier(threads)

    def fail(self, text):
        with self.lock:
            self.failures.append(text)
            print("FAIL " + text, flush=True)

    def thread(self, t, body):
        """the preamble of every worker thread, then body(t, stream); an exception is a failure line"""
        import torch

        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                self.F.use_torch_stream()
                body(t, s)
                s.synchronize()
        except threading.BrokenBarrierError:
            self.fail(f"thread {t}: a barrier broke (another thread did not arrive)")
        except BaseException:
            self.fail(f"thread {t}: {traceback.format_exc()}")
            self.barrier.abort()  # the others end at their next barrier instead of waiting for this thread

    def start(self, body, n=None):
        ths = [threading.Thread(target=self.thread, args=(t, body)) for t in range(n or self.threads)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()


def main_stream():
    import torch

    return torch.cuda.Stream()


def run_table(run, group):
    import torch

    F, T = run.F, run.threads
    names = sorted(set(hc.GROUPS[group]) | set(hc.phase_c_table(group)))
    plan = group == "look-ahead"
    if plan:  # process wide: once, before the threads start
        F.lib().faer_hip_debug_lu_plan(*(C.c_size_t(v) for v in LU_LA_PLAN))
    try:
        cases = {n: build_case(F, n) for n in names}
        torch.cuda.synchronize()
        # ---- A. the baseline: every case once, alone, on a non-blocking stream of the main thread
        base = {}
        S = main_stream()
        with torch.cuda.stream(S):
            F.use_torch_stream()
            for n in names:
                base[n] = run_case(F, cases[n], S)
                if cases[n].check is not None and not cases[n].check(base[n][0]):
                    run.fail(f"baseline {n}: not the outcome its own test expects")
            S.synchronize()
        F.use_torch_stream()
        if plan:  # the plan knob did change the driver (test_plu_lookahead): other rounding than the tuned plan's
            F.lib().faer_hip_debug_lu_plan(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))
            tuned = cases[hc.LU_LA].inputs["a"].clone()
            F.partial_piv_lu_factor_in_place(tuned)
            F.synchronize()
            if np.array_equal(tuned.cpu().numpy().view(np.int64), base[hc.LU_LA][0]["lu"].view(np.int64)):
                run.fail("the LU plan knob did not change the driver")
            del tuned
            F.lib().faer_hip_debug_lu_plan(*(C.c_size_t(v) for v in LU_LA_PLAN))
        torch.cuda.synchronize()
        sched = hc.schedule(group, T)
        barrier = run.barrier
        spans = [[None] * T for _ in sched]
        spans_b = {n: [None] * T for n in hc.GROUPS[group]}  # (the first run behind each barrier of phase B)

        def body(t, s):
            # ---- B. the same case on every thread at once
            for n in hc.GROUPS[group]:
                ready = [prepare(cases[n]) for _ in range(hc.RUNS[group])]  # the uploads before the barrier: the calls themselves overlap
                s.synchronize()
                barrier.wait(BARRIER_TIMEOUT)
                for r in range(hc.RUNS[group]):
                    try:
                        got, diag = run_case(F, cases[n], s, ready[r])
                        if r == 0:
                            spans_b[n][t] = cases[n].last_span[threading.get_ident()]
                        bad = compare(n, cases[n], base[n], got, diag, f"B thread {t} run {r} {n}")
                    except AssertionError as ex:
                        bad = f"B thread {t} run {r} {n}: {ex}"
                    if bad:
                        run.fail(bad)
            # ---- C. different cases at once
            for i, step in enumerate(sched):
                n = step[t]
                ready = prepare(cases[n])
                s.synchronize()
                barrier.wait(BARRIER_TIMEOUT)
                try:
                    got, diag = run_case(F, cases[n], s, ready)
                    spans[i][t] = cases[n].last_span[threading.get_ident()]
                    bad = compare(n, cases[n], base[n], got, diag, f"C step {i} thread {t} {n} beside {[c for c in step if c != n]}")
                except AssertionError as ex:
                    bad = f"C step {i} thread {t} {n}: {ex}"
                if bad:
                    run.fail(bad)

        run.start(body)
        run.info["cases"] = len(names)
        run.info["steps"] = len(sched)
        # the control: behind how many barriers of phase B (first run) and in how many steps of phase C two threads' calls were in flight
        # at the same time (host clock, from the call to the end of its stream's work); a child in which none were would have run its
        # cases one after the other
        both = lambda a, b: a is not None and b is not None and a[0] < b[1] and b[0] < a[1]
        overlapped = lambda rows: sum(any(both(sp[i], sp[j]) for i in range(T) for j in range(i)) for sp in rows)
        run.info["same_case_barriers"] = len(spans_b)
        run.info["overlapped_same_case"] = overlapped(spans_b.values())
        run.info["overlapped_steps"] = overlapped(spans)
    finally:
        if plan:
            F.lib().faer_hip_debug_lu_plan(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))


# ------------------------------------------------------------------------------------------ status belongs to the caller
def run_status(run):
    import torch

    F, T = run.F, run.threads
    bad_pivot = spd(np.random.default_rng(300), 300)
    bad_pivot[150, 150] = -1.0
    nan = rnd(np.random.default_rng(130), 130, 130)
    nan[17, 5] = np.nan
    rebuild = build_case(F, "lu_rebuild:f64")
    S = main_stream()
    with torch.cuda.stream(S):
        F.use_torch_stream()
        base = run_case(F, rebuild, S)
    F.use_torch_stream()
    torch.cuda.synchronize()

    def llt_role(t, s, ready, what):
        a = ready["a"]
        try:
            return f"{what}: no error, count {F.llt_factor_in_place(a)}"
        except F.LltError as e:
            return None if e.index == 150 else f"{what}: NonPositivePivot index {e.index}, not 150"

    def svd_role(t, s, ready, what):
        d = ready
        tag = F.svd(d["a"], d["s"][:, 0], d["u"], d["v"])
        return None if tag == F.SVD_NO_CONVERGENCE else f"{what}: svd tag {tag}, not NoConvergence"

    def lu_role(t, s, ready, what):
        got, diag = run_case(F, rebuild, s, ready)
        return compare("lu_rebuild:f64", rebuild, base, got, diag, what)

    roles = [llt_role, svd_role, lu_role][:T]
    inputs = {llt_role: {"a": bad_pivot}, svd_role: {"a": nan, "s": np.zeros((130, 1)), "u": np.zeros((130, 130)), "v": np.zeros((130, 130))},
              lu_role: rebuild.inputs}
    barrier = run.barrier

    def body(t, s):
        for r in range(hc.STATUS_ROUNDS):
            role = roles[(t + r) % T]
            ready = _fresh(inputs[role])
            s.synchronize()
            barrier.wait(BARRIER_TIMEOUT)
            try:
                bad = role(t, s, ready, f"E round {r} thread {t} {role.__name__}")
            except AssertionError as ex:
                bad = f"E round {r} thread {t} {role.__name__}: {ex}"
            s.synchronize()
            if bad:
                run.fail(bad)

    run.start(body)


# ------------------------------------------------------------------------------------------ thread lifetime
def run_lifetime(run):
    """G generations of 2 fresh threads; each thread runs the two cases on preallocated tensors, checks them, calls faer_hip_shutdown
    and ends.  info["free"][g]: free device memory after generation g (g = 0: before the first)"""
    import torch

    F = run.F
    cases = {n: build_case(F, n) for n in hc.LIFETIME_CASES}
    S = main_stream()
    base = {}
    with torch.cuda.stream(S):
        F.use_torch_stream()
        for n, c in cases.items():
            base[n] = run_case(F, c, S)
    F.use_torch_stream()
    # everything torch allocates, once: per thread slot the masters and the working buffers
    master = {n: _fresh(c.inputs) for n, c in cases.items()}
    work = [{n: {k: v.clone() for k, v in master[n].items()} for n in cases} for _ in range(2)]
    torch.cuda.synchronize()
    def once(t, s, what):
        for n, c in cases.items():
            for k, v in work[t][n].items():
                v.copy_(master[n][k], non_blocking=True)
            with Routes(F) as r:
                out = c.fn(work[t][n])
            s.synchronize()
            try:
                same_result(base[n][0], to_host(out), f"{what} {n}")
                assert {k: int(v) for k, v in r.hits.items() if v} == base[n][1]["routes"], f"{what} {n}: routes"
            except AssertionError as ex:
                run.fail(str(ex))

    # What is measured is what the LIBRARY keeps, so every generation asks the runtime for the same memory in the same order.  The runtime
    # carves small device allocations out of 2 MiB blocks of its own and keeps those blocks at their high-water mark; how many blocks
    # two pools need depends on how the two threads' allocations interleave, and with both threads allocating at once the generation
    # that met the worst packing was any of them.  So the threads of a generation fill their pools one after the other (in_turn), hold
    # them together at the barrier (both pools exist at the same time in EVERY generation) and then shut down at the same time.
    turn = threading.Semaphore(1)

    def in_turn(t, s, what):
        if not turn.acquire(timeout=BARRIER_TIMEOUT):
            raise threading.BrokenBarrierError
        try:
            once(t, s, what)
        finally:
            turn.release()

    def body(t, s):
        in_turn(t, s, f"lifetime thread {t}")
        run.barrier.wait(BARRIER_TIMEOUT)
        F.lib().faer_hip_shutdown()

    def body_reuse(t, s):  # a call after the shutdown, on the same thread
        in_turn(t, s, f"lifetime thread {t} before shutdown")
        run.barrier.wait(BARRIER_TIMEOUT)
        F.lib().faer_hip_shutdown()
        in_turn(t, s, f"lifetime thread {t} after shutdown")
        run.barrier.wait(BARRIER_TIMEOUT)
        F.lib().faer_hip_shutdown()

    # ... and what the runtime keeps per stream and per hardware queue, which is not the library's to free: torch creates its pool of 32
    # streams per device one by one on first use, and a hardware queue gets its scratch memory (about 16 MiB here) when the first kernel
    # with private memory runs on it.  So the main thread makes the same calls on every stream of torch's pool first.
    pool = [torch.cuda.Stream() for _ in range(32)]
    for s in pool:
        with torch.cuda.stream(s):
            F.use_torch_stream()
            once(0, s, "lifetime warm-up")
    F.use_torch_stream()
    torch.cuda.synchronize()
    # ... and what the runtime sets up for the first threads other than the main one: a generation that is not counted
    run.start(body, 2)
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info()[0]]
    for g in range(hc.LIFETIME_GENERATIONS):
        run.start(body, 2)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    run.info["free"] = free
    run.start(body_reuse, 2)
    torch.cuda.synchronize()
    run.info["free_after_reuse"] = torch.cuda.mem_get_info()[0]


def main(argv):
    import torch

    group, threads, out = argv[0], int(argv[1]), argv[2]
    torch.cuda.set_device(0)
    F = fa()
    F.lib().faer_hip_debug_qr_one_pass_columns.restype = C.c_long
    run = Run(F, threads)
    if group == "status":
        run_status(run)
    elif group == "lifetime":
        run_lifetime(run)
    else:
        run_table(run, group)
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump({"failures": run.failures, "info": run.info, "queues": os.environ.get("GPU_MAX_HW_QUEUES")}, f)
    print(f"worker {group} T={threads}: {len(run.failures)} failure(s)", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
