"""The case table and the phase C schedules of tests/test_gpu_host_threads.py, checked without a GPU."""
import itertools

import pytest

import host_threads_cases as hc
from test_gpu_stream_order import SMALL


def test_table_names_every_family():
    small = {c.split(":")[0] for c in hc.GROUPS["small-f64"]}
    assert small == set(SMALL)
    assert {c.split(":")[0] for c in hc.GROUPS["small-f32"]} == {f for f in SMALL if not f.startswith("dist")}
    assert all(c.endswith(":f64") for c in hc.GROUPS["small-f64"]) and all(c.endswith(":f32") for c in hc.GROUPS["small-f32"])
    # every look-ahead / QR / LU case
    for name in ("llt_la_3077:f64", "llt_step_kinds_5197:f64", "lu_la_3072:f64", "lu_600x5:f64", "lu_1000x1000:f64", "qr_20000x64_bs64:f32",
                 "qr_16500x17_bs1:f64", "qr_2100x800_bs192:f64", "qr_512x200_bs32:f64"):
        assert name in hc.ALL_CASES, name
    # every newer family
    newer = set(hc.GROUPS["newer-families"])
    assert {"clu_700:c64", "clu_5000x40:c64", "cmatmul_300x200x1000:c64", "ctrsm_poisoned_pool_sizes:c32"} <= newer
    for fam in ("chol_update", "evd_general", "gevd"):
        assert {f"{fam}:f64", f"{fam}:f32"} <= newer
    # each case belongs to a group that runs it on every thread at once (phase B)
    in_b = {c for g in hc.GROUPS.values() for c in g}
    assert set(hc.ALL_CASES) == in_b
    assert set(hc.GROUPS) == set(hc.RUNS)
    assert all(hc.RUNS[g] == 3 for g in ("small-f64", "small-f32", "default-queues"))
    assert all(hc.RUNS[g] == 2 for g in ("look-ahead", "llt-step-kinds", "qr", "newer-families"))
    # the default-queue pass: the small table in fp64 only, no look-ahead case
    assert hc.GROUPS["default-queues"] == hc.GROUPS["small-f64"]
    assert set(hc.LIFETIME_CASES) <= set(hc.GROUPS["small-f64"])


def test_equality_classes():
    allowed = {"lu_600x5:f64", "lu_la_3072:f64", "qr_20000x64_bs64:f32", "qr_16500x17_bs1:f64", "qr_2100x800_bs192:f64", "clu_5000x40:c64"}
    assert hc.BOUNDED_ALLOWED == allowed
    assert set(hc.BOUNDED) <= allowed
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in hc.BOUNDED.values())
    assert hc.PIVOTS == {"lu_1000x1000:f64"} and not (hc.PIVOTS & set(hc.BOUNDED))
    for case in hc.ALL_CASES:  # exactly one class each
        assert hc.equality_class(case) == ("bounded" if case in hc.BOUNDED else "pivots" if case in hc.PIVOTS else "bitwise")


@pytest.mark.parametrize("threads", [2, 3])
@pytest.mark.parametrize("group", sorted(hc.GROUPS))
def test_schedule(group, threads):
    sched = hc.schedule(group, threads)
    table = hc.phase_c_table(group)
    if len(table) < threads:
        assert sched == [] and group == "llt-step-kinds"
        return
    for step in sched:
        assert len(step) == threads and len(set(step)) == threads, step  # never the same case twice in a step
        assert set(step) <= set(table)
    assert {c for step in sched for c in step} == set(table)  # every case of the table runs beside another one
    if group != "look-ahead":
        for t in range(threads):  # every thread walks the whole table
            assert sorted(step[t] for step in sched) == sorted(table)
    assert sched == hc.schedule(group, threads)  # (deterministic: the child and the test build the same one)


@pytest.mark.parametrize("threads", [2, 3])
def test_schedule_brings_the_contended_cases_together(threads):
    contended = ["lu_la_3072:f64", "lu_600x5:f64", "qr_16500x17_bs1:f64", "qr_2100x800_bs192:f64", "clu_5000x40:c64", "llt_la_3077:f64"]
    assert sorted(hc.CONTENDED) == sorted(contended)
    met = set()
    for step in hc.schedule("look-ahead", threads):
        met |= {frozenset(p) for p in itertools.combinations(step, 2)}
    for a, b in itertools.combinations(contended, 2):
        assert frozenset((a, b)) in met, (a, b)
    for c in contended:
        assert frozenset((c, "tridiag:f64")) in met or frozenset((c, "fplu:f64")) in met, c
        assert frozenset((c, "matmul_wide:f64")) in met, c
    # the places rotate: no contended case is always the same thread's
    for c in contended:
        assert len({step.index(c) for step in hc.schedule("look-ahead", threads) if c in step}) > 1, c
