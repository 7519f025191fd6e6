"""CPU tests of the complex level-3 boundary (include/faer_hip.h: matmul, matmul_triangular and the four triangular solves for
c32 / c64): the prototypes are declared, both spellings are exported, the argument checks that precede any staging abort with their
own messages (in a child process: the boundary's error convention is abort()), a family that stays real-only still ends in its
stub -- and the two error bounds of the GPU tests are reachable by a plain numpy reference on the same inputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import complex_cases as cc
from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("matmul", "matmul_triangular", "solve_triangular_lower_in_place", "solve_triangular_upper_in_place",
            "solve_unit_triangular_lower_in_place", "solve_unit_triangular_upper_in_place")
NAMES = [f"libfaer_v0_23_{f}_{s}" for f in FAMILIES for s in ("c32", "c64")]


def test_header_declares_the_twelve_prototypes():
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    assert len(NAMES) == 12
    for name in NAMES:
        assert re.search(r"FAER_HIP_API\s+void\s+" + name + r"\(", hdr), name
        # the argument list is the f64 one
        args = re.search(name + r"\(([^;]*)\);", hdr).group(1)
        args64 = re.search(name[:-3] + r"f64\(([^;]*)\);", hdr).group(1)
        assert args == args64, name


def test_both_spellings_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", fa().LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in NAMES:
        assert name in exported, name
        assert name.replace("v0_23", "v0_24") in exported, name


def test_python_mirror_knows_the_complex_dtypes():
    F = fa()
    assert F._dtype_suffix(np.zeros((1, 1), np.complex64))[0] == "c32" and F._dtype_suffix(np.zeros((1, 1), np.complex128))[0] == "c64"
    al = F._dtype_suffix(np.zeros((1, 1), np.complex64))[1](2 - 1j)
    assert (al.re, al.im) == (2.0, -1.0)
    with pytest.raises(TypeError, match="c32 / c64"):
        F._dtype_suffix(np.zeros((1, 1), np.int32))


def child(body):
    """runs `body` (F = the package, np, C = ctypes in scope) in a fresh interpreter; returns (returncode, stderr)"""
    code = ("import sys\nsys.path.insert(0, %r)\nimport ctypes as C\nimport numpy as np\nfrom gpu_util import fa\nF = fa()\nF.lib()\n" % os.path.join(ROOT, "tests")) + body
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stderr


def test_matmul_c64_checks_dimensions_before_anything_else():
    rc, err = child("a = np.zeros((3, 4), np.complex128, order='F'); b = np.zeros((5, 2), np.complex128, order='F')\n"
                    "c = np.zeros((3, 2), np.complex128, order='F')\nF.matmul(c, F.ACCUM_REPLACE, a, b, 1.0)\nprint('returned')\n")
    assert rc == -6, (rc, err)
    assert "matmul: dimension mismatch" in err and "scalar type not implemented" not in err, err


def test_trsm_c32_checks_dimensions_before_anything_else():
    rc, err = child("t = np.eye(3, dtype=np.complex64, order='F'); x = np.zeros((4, 2), np.complex64, order='F')\n"
                    "F.solve_lower_triangular_in_place(t, x, conj=True)\n")
    assert rc == -6, (rc, err)
    assert "triangular solve: dimension mismatch" in err, err


def test_real_only_family_still_ends_in_its_stub():
    rc, err = child("F.lib().libfaer_v0_23_llt_factor_in_place_c64()\n")
    assert rc == -6, (rc, err)
    assert "libfaer_v0_23_llt_factor_in_place_c64: scalar type not implemented" in err, err


def test_complex_gemm_refuses_diag():
    rc, err = child("a = np.zeros((3, 3), np.complex128, order='F'); d = np.ones(3, np.complex128)\n"
                    "F.gemm(a.copy(order='F'), F.DST_FULL, F.ACCUM_REPLACE, a, a, 1.0, diag=d)\n")
    assert rc == -6, (rc, err)
    assert "row_idx / col_idx / diag are not implemented for complex scalars" in err, err


# ---- the yardsticks themselves: a plain numpy reference in the working precision stays inside both bounds
@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("m,n,k", cc.MATMUL_SHAPES)
def test_numpy_product_is_within_the_product_bound(m, n, k, dtype):
    a, b, c0, _, _ = cc.matmul_case(m, n, k, dtype)
    for mode, alpha in cc.MATMUL_MODES:
        ref, bound = cc.matmul_ref_and_bound(m, n, k, dtype, mode, alpha)
        got = np.dtype(dtype).type(alpha) * (a @ b) + (c0 if mode == "add" else 0)
        assert got.dtype == np.dtype(dtype)
        assert (np.abs(cc.ext(got) - ref) <= bound).all(), (mode, float((np.abs(cc.ext(got) - ref) - bound).max()))


@pytest.mark.parametrize("dtype", cc.CDTYPES)
@pytest.mark.parametrize("n", cc.TRSM_SIZES)
def test_numpy_substitution_is_within_the_solve_bound(n, dtype):
    for nrhs in cc.TRSM_NRHS:
        for triangle, unit in cc.TRSM_VARIANTS:
            t, b = cc.trsm_case(n, nrhs, dtype, triangle, unit)
            for conj in (False, True):
                x = cc.substitute(t, b, triangle, unit, conj)
                assert x.dtype == np.dtype(dtype)
                assert cc.tri_backward_error(t, x, b, conj) <= 1.0, (nrhs, triangle, unit, conj)


def test_exact_cases_are_exact_and_conj_matters():
    for dtype in cc.CDTYPES:
        for triangle, unit in cc.TRSM_VARIANTS:
            sols = []
            for conj in (False, True):
                t, b, x0 = cc.exact_trsm_case(40, 33, dtype, triangle, unit, conj)
                assert np.array_equal(cc.substitute(t, b, triangle, unit, conj), x0)
                sols.append(cc.substitute(t, b, triangle, unit, not conj))
                assert not np.array_equal(sols[-1], x0)
