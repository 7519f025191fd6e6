"""The leaf bodies of csrc/ctrtri_core.h on the host: tests/host/ctrtri_host.cpp inverts a matrix with them (reciprocal once per
diagonal entry, substitution on the sub-blocks, doubling inside a leaf, block products above it -- the schedule of ctrtri.hip in plain
loops) and the result is held against the numpy restatement of the reference's recursion (tests/complex_tri_inverse_ref.py).  No GPU.

Checked per case: the residual of the result is at most HOST_FACTOR times the yardstick's (floored at eps, see the reference module);
what must not be written is bit-identical to what came in; the exact case comes back exactly.  HOST_FACTOR = 4: both schedules are
backward-stable inversions of the same well-conditioned matrix and differ in the order of their sums and in the reciprocal
(conj(z) / |z|^2 here, a quotient there: two more roundings per diagonal entry); the device test records its own ratios."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import complex_tri_inverse_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ctrtri_host.cpp")
INC = os.path.join(ROOT, "faer-rs_amd", "csrc")
NP = {"c64": np.complex128, "c32": np.complex64}
SIZES = (1, 2, 15, 17, 33, 63, 64, 65, 129, 197)
HOST_FACTOR = 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = tmp_path_factory.mktemp("ctrtri_host") / "ctrtri_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", str(out)], check=True, capture_output=True, text=True)
    return str(out)


def run(exe, tmp_path, dtype, t, unit):
    """lower inverse of t through the host program; t's other entries travel along and must come back untouched"""
    n = t.shape[0]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    flat = np.empty(2 * n * n)
    flat[0::2] = t.real.ravel(order="F")
    flat[1::2] = t.imag.ravel(order="F")
    np.concatenate([[float(n), float(unit)], flat]).tofile(fin)
    subprocess.run([exe, dtype, str(fin), str(fout)], check=True)
    o = np.fromfile(fout)
    return (o[0::2] + 1j * o[1::2]).reshape(n, n, order="F").astype(NP[dtype])


@pytest.mark.parametrize("dtype", ["c64", "c32"])
@pytest.mark.parametrize("unit", [False, True])
def test_host_bodies_against_the_restatement(exe, tmp_path, dtype, unit):
    for n in SIZES:
        t, tp, _, r_ref = ref.case(n, NP[dtype], "lower", unit)
        got = run(exe, tmp_path, dtype, tp, unit)
        keep = ~ref.written_mask(n, "lower", unit)
        assert np.isnan(got[keep]).all(), n  # the poison came back: nothing outside the triangle was produced from it or written
        r = ref.residual(t, got, "lower", unit)
        assert r <= HOST_FACTOR * ref.yardstick(r_ref, NP[dtype]), (n, r, r_ref)


@pytest.mark.parametrize("dtype", ["c64", "c32"])
@pytest.mark.parametrize("unit", [False, True])
def test_host_bodies_are_exact_on_the_exact_case(exe, tmp_path, dtype, unit):
    for n in (65, 197):
        t, w = ref.exact_case(n, NP[dtype], "lower", unit)
        got = run(exe, tmp_path, dtype, t, unit)
        m = ref.written_mask(n, "lower", unit)
        assert np.array_equal(got[m], w[m]), n
