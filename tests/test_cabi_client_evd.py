"""A compiled C client of the general EVD (tests/cabi_client/evd_client.c): against the reference's own faer-ffi/faer.h where
that tree is present (links against libfaer_hip.so and runs its host-only part: constructors, function pointers, scratch
query), and against include/faer_hip.h on the GPU, where it decomposes a small host-resident matrix."""
import os
import shutil
import subprocess

import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FFI = os.path.join(os.environ.get("FAER_REFERENCE", "/root/reference"), "faer-ffi")
SRC = os.path.join(ROOT, "tests", "cabi_client", "evd_client.c")


def compile_client(out, ref_header):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    libdir = os.path.dirname(fa().LIB_PATH)
    inc = [f"-I{REF_FFI}", "-DEVD_CLIENT_REF_HEADER"] if ref_header else [f"-I{os.path.join(ROOT, 'include')}"]
    subprocess.run([cc, "-std=c11", "-O1", "-Wall", "-Werror", *inc, SRC, "-o", str(out), f"-L{libdir}", "-lfaer_hip", "-lm",
                    f"-Wl,-rpath,{libdir}"], check=True, capture_output=True, text=True)
    return str(out)


def test_client_against_the_reference_header_links_and_runs_host_only(tmp_path):
    if not os.path.exists(os.path.join(REF_FFI, "faer.h")):
        pytest.skip("reference faer.h not available")
    exe = compile_client(tmp_path / "evd_client_ref", True)
    r = subprocess.run([exe, "host-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "host-only ok" in r.stdout, r.stderr


def test_client_against_the_project_header_runs_host_only(tmp_path):
    exe = compile_client(tmp_path / "evd_client", False)
    r = subprocess.run([exe, "host-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "host-only ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_client_computes_on_the_gpu(tmp_path):
    exe = compile_client(tmp_path / "evd_client", False)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "evd_client ok" in r.stdout, (r.stdout, r.stderr)
