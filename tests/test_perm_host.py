"""CPU test of the host-only part of csrc/perm.h: perm_from_transpositions -- the loop every pivoted factorization ends with -- in
a stand-alone program (tests/perm_host.cpp, host compiler, no HIP header) against a NumPy restatement of the same loop."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
BIN = os.path.join(BUILD, "perm_host")


def build_program():
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "perm_host.cpp")
    hdr = os.path.join(ROOT, "faer-rs_amd", "csrc", "perm.h")
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", BIN, src])
    return BIN


def restated(n, starts, records):
    """identity, the swaps (j <-> block start of j + record j) in order, how many moved something, the inverse"""
    perm, count = np.arange(n), 0
    for j, r in enumerate(records):
        p = max(s for s in starts if s <= j) + r
        assert j <= p < n
        if p != j:
            perm[[j, p]] = perm[[p, j]]
            count += 1
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    return perm, inv, count


N = 11
CASES = {
    "identity": ([0], list(range(N))),
    "single swap": ([0], [0, 1, 7] + list(range(3, N))),
    "chain to the last row": ([0], [N - 1] * N),
    "fewer records than rows": ([0], [4, 4, 2]),
    # two blocks, starting at rows 0 and 6: a record counts from the first row of its block
    "block relative": ([0, 6], [3, 1, 5, 3, 4, 5] + [2, 1, 4, 3, 4]),
}


@pytest.mark.parametrize("name", CASES)
def test_perm_from_transpositions_matches_the_restated_loop(name):
    starts, records = CASES[name]
    out = subprocess.run([build_program()] + [str(v) for v in [N, len(starts)] + starts + [len(records)] + records], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    perm, inv, count = restated(N, starts, records)
    assert [int(v) for v in out[0].split()] == list(perm) and [int(v) for v in out[1].split()] == list(inv) and int(out[2]) == count
    assert sorted(perm) == list(range(N)) and (name == "identity") == (count == 0)


def test_a_record_above_its_row_or_past_the_end_is_fatal():
    for records in ([1, 0], [0, N]):
        r = subprocess.run([build_program(), str(N), "1", "0", str(len(records))] + [str(v) for v in records], capture_output=True, text=True)
        assert r.returncode != 0 and "perm_host: pivot record out of range" in r.stderr
