"""What the scratch queries and params getters of the boundary return, against a recorded snapshot (no GPU).

include/faer_hip.h pins every name and signature (a conflicting definition does not compile) but not what the small bodies of
csrc/api.hip, lblt.hip and piv_llt.hip return.  tests/abi_scratch_snapshot.json holds those answers as tools/dump_abi_scratch.py
printed them from a build of the commit named in its "generated_from" -- the parent of the change that restructured the outer
boundary of api.hip -- so a wrapper that lost an argument, swapped two, or took sizeof of the wrong type fails here.  The
enumeration comes from the header: a new scratch query without a recorded answer fails too (regenerate the snapshot from a build
that does NOT contain the change under review)."""
import json
import os
import sys

from gpu_util import ROOT, fa

sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import dump_abi_scratch
finally:
    sys.path.pop(0)

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_scratch_snapshot.json")


def recorded():
    return json.load(open(SNAPSHOT))["entries"]


def differences(got, want):
    return {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}


def test_header_enumeration_is_not_empty():
    hdr = dump_abi_scratch.Header()
    names = hdr.queries()
    layouts = [n for n in names if hdr.protos[n][0] == "FaerLayout"]
    # every family has both kinds, for f32 and f64 at least; index-typed and complex ones come on top
    assert len(layouts) >= 100 and len(names) - len(layouts) >= 40, (len(layouts), len(names))
    assert all(n.startswith("libfaer_v0_23_") or n.startswith("faer_hip_") for n in names)


def test_every_query_and_getter_returns_what_the_snapshot_recorded():
    got, want = dump_abi_scratch.dump(fa().LIB_PATH), recorded()
    missing = sorted(set(got) - set(want))
    assert not missing, f"declared in the header, not in the snapshot: {missing}"
    gone = sorted(set(want) - set(got))
    assert not gone, f"in the snapshot, no longer declared in the header: {gone}"
    diff = differences(got, want)
    assert not diff, f"(got, recorded): {diff}"


def test_v0_24_spellings_return_the_same():
    got, want = dump_abi_scratch.dump(fa().LIB_PATH, spelling="v0_24"), recorded()
    # faer.hpp spells every entry point v0_24 (csrc/abi_compat.c): each libfaer_* query has its alias
    expected = {k for k in want if k.startswith("libfaer_v0_23_")}
    assert set(got) == expected, sorted(set(got) ^ expected)
    diff = differences(got, {k: want[k] for k in expected})
    assert not diff, f"(v0_24, recorded): {diff}"
