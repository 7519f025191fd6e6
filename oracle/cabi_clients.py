"""Recipe of the compiled C-ABI clients (tests/cabi_client/): built against the reference's own faer-ffi/faer.h and faer.hpp,
linked against faer-rs_amd/libfaer_hip.so.  The binaries land in oracle/_ref/cabi_client/ (git-ignored); the reference's
headers are read from `ref_dir` and nothing of them is kept.  __graft_entry__.build() runs this where the reference tree
is available (through tests/test_cabi_client.build_clients); tests/test_cabi_client.py runs the binaries."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "oracle", "_ref", "cabi_client")
LIBDIR = os.path.join(ROOT, "faer-rs_amd")
NAMES = ("ref_client", "hpp_client")


def binaries():
    return [os.path.join(OUT, n) for n in NAMES]


def build(ref_dir):
    """returns the two binaries; raises CalledProcessError with the compiler output on a layout / prototype mismatch"""
    ffi = os.path.join(ref_dir, "faer-ffi")
    os.makedirs(OUT, exist_ok=True)
    rpath = "-Wl,-rpath,$ORIGIN/../../../faer-rs_amd"  # oracle/_ref/cabi_client -> faer-rs_amd
    ref_bin, hpp_bin = binaries()
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", f"-I{ffi}", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "cabi_client", "ref_client.c"), "-o", ref_bin, f"-L{LIBDIR}", "-lfaer_hip", "-lm",
                    rpath], check=True, capture_output=True, text=True)
    # faer.hpp spells libfaer_v0_24_* but faer.h declares libfaer_v0_23_* (header drift in the reference): the C++
    # client compiles against a GENERATED copy of faer.h with the v0_24 spelling, in a temporary directory
    with tempfile.TemporaryDirectory() as hpp:
        hdr = open(os.path.join(ffi, "faer.h")).read().replace("libfaer_v0_23_", "libfaer_v0_24_")
        open(os.path.join(hpp, "faer.h"), "w").write(hdr)
        for f in ("faer.hpp", "quad.hpp"):
            with open(os.path.join(ffi, f)) as src, open(os.path.join(hpp, f), "w") as dst:
                dst.write(src.read())
        subprocess.run(["g++", "-std=c++20", "-O1", f"-I{hpp}", os.path.join(ROOT, "tests", "cabi_client", "hpp_client.cpp"),
                        "-o", hpp_bin, f"-L{LIBDIR}", "-lfaer_hip", rpath], check=True, capture_output=True, text=True)
    return ref_bin, hpp_bin
