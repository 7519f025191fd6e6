"""A compiled C client of the generalized EVD (tests/cabi_client/gevd_client.c), written against the reference's own faer-ffi/faer.h
and linked against libfaer_hip.so, like the clients of tests/test_cabi_client.py.  Building needs the reference tree
(FAER_REFERENCE); the binary lands next to the other clients in oracle/_ref/cabi_client/ (git-ignored, built by
__graft_entry__.build()), where the host-only test runs it and the -m gpu test runs it in `compute` mode."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FAER_REFERENCE", "/root/reference")
LIBDIR = os.path.join(ROOT, "faer-rs_amd")
OUT = os.path.join(ROOT, "oracle", "_ref", "cabi_client")
BIN = os.path.join(OUT, "gevd_client")


def build_client():
    """compiles and links the client against the reference's header; raises CalledProcessError with the compiler's output"""
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", f"-I{os.path.join(REF, 'faer-ffi')}", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "cabi_client", "gevd_client.c"), "-o", BIN, f"-L{LIBDIR}", "-lfaer_hip", "-lm",
                    "-Wl,-rpath,$ORIGIN/../../../faer-rs_amd"], check=True, capture_output=True, text=True)
    return BIN


def test_client_compiles_links_and_runs_host_only():
    if os.path.exists(os.path.join(REF, "faer-ffi", "faer.h")):
        try:
            build_client()
        except subprocess.CalledProcessError as e:  # show the compiler's message (e.g. the failing _Static_assert)
            pytest.fail(e.stderr[-4000:])
    elif not os.path.exists(BIN):
        pytest.skip("neither the reference tree nor the client binary built by __graft_entry__.build() is available")
    r = subprocess.run([BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "ok (host-only)" in r.stdout


@pytest.mark.gpu
def test_client_computes_on_the_gpu():
    if not os.path.exists(BIN):
        pytest.skip("the client binary is built where the reference tree is available (__graft_entry__.build())")
    r = subprocess.run([BIN, "compute"], capture_output=True, text=True, timeout=300)
    if r.returncode == 2 and "no gfx950 device" in (r.stdout + r.stderr):
        pytest.skip("no gfx950 device visible to the client")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok (compute)" in r.stdout
