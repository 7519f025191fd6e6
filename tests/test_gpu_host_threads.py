"""Independent library calls from 2 and 3 concurrent host threads of one process (the entry points are
thread safe, per-thread stream and scratch; csrc/common.h: everything mutable is thread_local).

Each test runs ONE fresh child process (tests/host_threads_worker.py, through a launcher written to tmp_path) and reads its verdicts
back.  Every worker thread has a non-blocking torch stream of its own and waits for that stream only.  Phases of a child:
  A  the main thread runs every case of the group once, alone: outputs, the calling thread's counters (debug_*_last, the one-pass QR
     column count, the GEMM / TRSM route counts);
  B  the T threads meet at a barrier and run the same case on fresh copies of the same inputs, R times each;
  C  different cases at once (host_threads_cases.schedule; the look-ahead group's schedule brings every pair of the cases that own
     internal streams or cooperative panel kernels together, and each of them with a level-2 family and the wide product);
  D  in B and C each thread's counters, read after its own call, equal the baseline's of that case;
  E  (group "status") at one barrier: a Cholesky with a bad pivot at 150, an SVD of a matrix with a NaN, a good LU with its solves --
     every thread gets its own outcome.
Results are compared bit for bit with the baseline (host_threads_cases.equality_class: LU 1000 x 1000 by pivots and the bound of
test_gpu_stream_order.test_plu, like that test).  The children run with GPU_MAX_HW_QUEUES=8 like tests/test_gpu_dist_threads.py; the
last test repeats the fp64 small table with two threads at the inherited setting (T threads hold up to 4 T streams).

A child that aborts, faults or runs into its limit fails its test with the tail of its output."""
import json
import os
import subprocess
import sys

import pytest

import host_threads_cases as hc
from test_gpu_factor import LLT_STEP_KINDS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

LAUNCHER = r'''
import sys
sys.path.insert(0, sys.argv[1])
import host_threads_worker
host_threads_worker.main(sys.argv[2:])
'''

# seconds: the child's start-up (python, torch, the library: about 10 s) and its work, several times over; not a measurement
TIMEOUT = {"small-f64": 240, "small-f32": 240, "default-queues": 240, "look-ahead": 300, "llt-step-kinds": 240, "qr": 240, "newer-families": 240,
           "status": 180, "lifetime": 180}


def run_child(tmp_path, group, threads, queues="8"):
    script, out = tmp_path / "launcher.py", tmp_path / "out.json"
    script.write_text(LAUNCHER)
    env = dict(os.environ, FAER_HIP_VERBOSE="1", **hc.ENV.get(group, {}))
    if group == "llt-step-kinds":
        env.update(LLT_STEP_KINDS)
    if queues is not None:
        env["GPU_MAX_HW_QUEUES"] = queues
    p = subprocess.run([sys.executable, str(script), HERE, group, str(threads), str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=TIMEOUT[group])
    text = p.stdout.decode(errors="replace")
    said = [line for line in text.splitlines() if line.startswith("faer_hip:")]
    if said:  # which fallback ran, if any (FAER_HIP_VERBOSE)
        print(f"{group} T={threads}: the library said\n  " + "\n  ".join(sorted(set(said))))
    assert p.returncode == 0, f"the child exited with {p.returncode}\n" + text[-3000:]
    res = json.loads(out.read_text())
    assert res["failures"] == [], "\n".join(res["failures"][:20]) + "\n--- the library said:\n" + "\n".join(sorted(set(said)))
    return res


@pytest.mark.parametrize("threads", hc.THREAD_COUNTS)
@pytest.mark.parametrize("group", ["small-f64", "small-f32", "look-ahead", "llt-step-kinds", "qr", "newer-families"])
def test_concurrent_calls(tmp_path, group, threads):
    res = run_child(tmp_path, group, threads)
    assert res["queues"] == "8"
    # the control (host clock, no timing claim): some calls of each phase were in flight at the same time
    info = res["info"]
    print(f"{group} T={threads}: two calls in flight at once behind {info['overlapped_same_case']} of {info['same_case_barriers']} barriers of "
          f"phase B and in {info['overlapped_steps']} of {info['steps']} steps of phase C")
    assert info["same_case_barriers"] == len(hc.GROUPS[group]) > 0
    assert info["overlapped_same_case"] > 0, "phase B ran its calls one after the other: nothing there was concurrent"
    if group != "llt-step-kinds":  # (one case: phases A and B only)
        assert info["steps"] == len(hc.schedule(group, threads)) > 0
        assert info["overlapped_steps"] > 0, "phase C ran its cases one after the other: nothing there was concurrent"


@pytest.mark.parametrize("threads", hc.THREAD_COUNTS)
def test_status_belongs_to_the_caller(tmp_path, threads):
    run_child(tmp_path, "status", threads)


def test_thread_lifetime(tmp_path):
    """8 generations of 2 fresh threads; each thread runs llt_rebuild and matmul_split_k (fp64) on preallocated tensors, checks them bit for
    bit, calls faer_hip_shutdown and ends.  Free device memory after generation 8 is no lower than after generation 2 by more than the
    drop of generation 1 alone (one set of pools: the slack for allocator granularity); then two threads make the same calls again
    AFTER their shutdown.

    Measured (MI355X, torch.cuda.mem_get_info, bytes lost per generation).  With a ctx_shutdown() that keeps the calling thread's
    pool, as it did: [4194304, 4194304, 2097152, 4194304, 4194304, 4194304, 4194304, 2097152] -- 20 MiB between generations 2 and 8
    against a slack of 4 MiB: growth with every generation, which this test fails.  With the pool freed: [0, 0, 0, 0, 0, 0, 0, 0],
    and the same free memory after the calls that follow a shutdown.

    The figure is the library's share only because the child keeps the runtime's own memory still (host_threads_worker.run_lifetime):
    it first makes the same calls on every stream of torch's pool (a hardware queue gets 16 MiB of scratch memory of the runtime's
    when the first kernel with private memory runs on it), then runs one generation that is not counted, and the two threads of a
    generation fill their pools one after the other before they hold them together and shut down at the same time -- the runtime
    carves small allocations out of 2 MiB blocks that it keeps at their high-water mark, and with both threads allocating at once the
    generation that met the worst packing, and lost one block, was any of the eight."""
    res = run_child(tmp_path, "lifetime", 2)
    free = res["info"]["free"]
    assert len(free) == hc.LIFETIME_GENERATIONS + 1
    drops = [free[g] - free[g + 1] for g in range(hc.LIFETIME_GENERATIONS)]
    print(f"free device memory before generation 1: {free[0]}; drop per generation: {drops}; after the calls that follow a shutdown: "
          f"{res['info']['free_after_reuse']}")
    slack = max(drops[0], 0)
    assert free[hc.LIFETIME_GENERATIONS] >= free[2] - slack, (drops, slack)
    assert res["info"]["free_after_reuse"] >= free[2] - slack, (res["info"]["free_after_reuse"], free[2], slack)


def test_default_hardware_queues(tmp_path):
    """the fp64 small table with two threads at the inherited GPU_MAX_HW_QUEUES (the runtime's default is 4): eight streams of the
    process share them.  Runs last"""
    run_child(tmp_path, "default-queues", 2, queues=None)
