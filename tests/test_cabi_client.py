"""Compiled clients of the drop-in boundary (VERDICT r01 "next round" item 3).

tests/cabi_client/ref_client.c is written against the reference's own faer-ffi/faer.h: struct layouts are
_Static_assert-ed against include/faer_hip.h, the `libfaer_v0_23_*` prototypes it calls are the reference's, and it
links against libfaer_hip.so.  tests/cabi_client/hpp_client.cpp does the same through the reference's C++ wrapper
faer-ffi/faer.hpp (v0_24 spelling + six-scalar dispatch tables => csrc/abi_compat.c).  Building needs the
reference tree (FAER_REFERENCE); the recipe is oracle/cabi_clients.py, the binaries land in oracle/_ref/cabi_client/
(git-ignored, built by __graft_entry__.build()), where the host-only test runs them whether or not the reference is at hand
and the -m gpu test runs them in `compute` mode."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FAER_REFERENCE", "/root/reference")
LIBDIR = os.path.join(ROOT, "faer-rs_amd")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cabi_clients  # noqa: E402

OUT = cabi_clients.OUT


def build_clients():
    """returns the two binaries (oracle/cabi_clients.build against the reference tree REF)"""
    return cabi_clients.build(REF)


def test_clients_compile_link_and_run_host_only():
    """compiled and linked here when the reference tree is at hand, else the binaries __graft_entry__.build() made are run"""
    bins = cabi_clients.binaries()
    if os.path.exists(os.path.join(REF, "faer-ffi", "faer.h")):
        try:
            bins = build_clients()
        except subprocess.CalledProcessError as e:  # show the compiler's message (e.g. the failing _Static_assert)
            pytest.fail(e.stderr[-4000:])
    elif not all(os.path.exists(b) for b in bins):
        pytest.skip("neither the reference tree nor client binaries built by __graft_entry__.build() are available")
    for b in bins:
        r = subprocess.run([b], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "ok (host-only)" in r.stdout


def test_abi_compat_is_up_to_date(tmp_path):
    """csrc/abi_compat.c is generated from include/faer_hip.h: a fresh generation (into a temporary file -- the tracked
    file is never rewritten by the test run) must be identical"""
    path = os.path.join(LIBDIR, "csrc", "abi_compat.c")
    fresh = str(tmp_path / "abi_compat.c")
    subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_abi_compat.py"), fresh], check=True, capture_output=True)
    assert open(fresh).read() == open(path).read()


def test_v024_aliases_and_stubs_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libfaer_hip.so")], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    v23 = {s for s in syms if s.startswith("libfaer_v0_23_") and s.endswith(("_f32", "_f64"))}
    assert len(v23) > 200
    for s in v23:
        assert s.replace("v0_23", "v0_24") in syms
        base = s.rsplit("_", 1)[0]
        for suf in ("fx128", "c32", "c64", "cx128"):
            assert f"{base}_{suf}" in syms and f"{base.replace('v0_23', 'v0_24')}_{suf}" in syms


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ref_client", "hpp_client"])
def test_clients_compute_on_the_gpu(name):
    b = os.path.join(OUT, name)
    if not os.path.exists(b):
        pytest.skip("client binaries are built where the reference tree is available (__graft_entry__.build())")
    r = subprocess.run([b, "compute"], capture_output=True, text=True, timeout=300)
    if r.returncode == 2 and "no gfx950 device" in (r.stdout + r.stderr):
        pytest.skip("no gfx950 device visible to the client")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok (compute)" in r.stdout
