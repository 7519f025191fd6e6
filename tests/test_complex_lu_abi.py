"""CPU tests of the complex partial-pivot LU boundary (include/faer_hip.h: PartialPivLuParams, factor, solve and transpose solve for
{u32, u64} x {c32, c64}): the prototypes are declared with the f64 argument lists, both spellings are exported, the parameter getter
and the scratch queries answer, the argument checks that precede any staging abort with their own messages (in a child process),
inverse stays a stub -- and the yardsticks of tests/test_gpu_complex_lu.py are reachable by the plain numpy restatement on the
shapes that file uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import complex_lu_ref as ref
from gpu_util import fa
from test_complex_abi import child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = ("u32", "u64")
SUF = ("c32", "c64")
FAMILIES = ("partial_piv_lu_factor_in_place_scratch", "partial_piv_lu_factor_in_place", "partial_piv_lu_solve_in_place_scratch",
            "partial_piv_lu_solve_in_place", "partial_piv_lu_solve_transpose_in_place_scratch", "partial_piv_lu_solve_transpose_in_place")
NAMES = [f"libfaer_v0_23_{f}_{i}_{s}" for f in FAMILIES for i in IDX for s in SUF] + [f"libfaer_v0_23_PartialPivLuParams_{s}" for s in SUF]


def test_header_declares_the_prototypes_with_the_f64_argument_lists():
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    assert len(NAMES) == 26
    for name in NAMES:
        decl = re.search(r"FAER_HIP_API\s+(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        decl64 = re.search(r"FAER_HIP_API\s+(\w+)\s+" + name[:-3] + r"f64\(([^;]*)\);", hdr)
        assert decl and decl64, name
        assert decl.groups() == decl64.groups(), name


def test_both_spellings_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", fa().LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in NAMES + ["faer_hip_debug_clu_shape", "faer_hip_debug_clu_last"]:
        assert name in exported, name
        if name.startswith("libfaer"):
            assert name.replace("v0_23", "v0_24") in exported, name


def test_params_scratch_queries_and_shape():
    F = fa()
    L = F.lib()
    p64, pc = L.libfaer_v0_23_PartialPivLuParams_f64(), L.libfaer_v0_23_PartialPivLuParams_c64()
    assert [getattr(pc, f) for f, _ in pc._fields_] == [getattr(p64, f) for f, _ in p64._fields_]
    for it in IDX:
        for suf, isz in (("c32", 8), ("c64", 16)):
            for name in ("partial_piv_lu_solve_in_place_scratch", "partial_piv_lu_solve_transpose_in_place_scratch"):
                fn = getattr(L, f"libfaer_v0_23_{name}_{it}_{suf}")
                assert fn(C.c_size_t(0), C.c_size_t(7), F.PAR_SEQ).len_bytes == 0
                assert fn(C.c_size_t(300), C.c_size_t(33), F.PAR_SEQ).len_bytes >= 300 * 33 * isz
            fn = getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_{it}_{suf}")
            assert fn(C.c_size_t(0), C.c_size_t(0), F.PAR_SEQ, pc).len_bytes == 0
            assert fn(C.c_size_t(300), C.c_size_t(64), F.PAR_SEQ, pc).len_bytes >= 64 * (4 if it == "u32" else 8)
    for dt in (np.complex64, np.complex128):
        w, leaf = F.debug_clu_shape(dt)
        assert 1 <= w <= 64 and leaf >= w
        assert 2 * w * leaf * np.dtype(dt).itemsize // 2 <= 160 * 1024  # the two planes of the tallest leaf fit the LDS of a CU
    assert F.debug_clu_shape(np.complex64)[1] >= F.debug_clu_shape(np.complex128)[1]
    with pytest.raises(TypeError, match="c32 / c64"):
        F._dtype_suffix(np.zeros((1, 1), np.int32))


def test_solve_checks_dimensions_before_anything_else():
    for transpose in (False, True):
        rc, err = child("lu = np.eye(3, dtype=np.complex128, order='F'); x = np.zeros((4, 2), np.complex128, order='F')\n"
                        "p = np.arange(3, dtype=np.uint64)\n"
                        f"F.partial_piv_lu_solve_in_place(lu, p, p, x, transpose={transpose}, conj=True)\nprint('returned')\n")
        assert rc == -6, (rc, err)
        assert "partial_piv_lu solve: dimension mismatch" in err and "scalar type not implemented" not in err, err


def test_solve_checks_the_permutation_slice_before_anything_is_staged():
    # the slice the solve does not use is checked first: perm_bwd of the plain solve
    rc, err = child("lu = np.eye(3, dtype=np.complex64, order='F'); x = np.zeros((3, 2), np.complex64, order='F')\n"
                    "p = np.arange(3, dtype=np.uint32); L = F.lib()\n"
                    "L.libfaer_v0_23_partial_piv_lu_solve_in_place_u32_c32(F._mat(lu), F._mat(lu), C.c_int(0), F.SliceRef(p.ctypes.data, 3),\n"
                    "    F.SliceRef(p.ctypes.data, 2), F._mat(x, F.MatMut), F.PAR_SEQ, F.MemAlloc(None, 0))\nprint('returned')\n")
    assert rc == -6, (rc, err)
    assert "partial_piv_lu solve: a permutation slice is too short" in err and "scalar type not implemented" not in err, err


def test_inverse_still_ends_in_its_stub():
    rc, err = child("F.lib().libfaer_v0_23_partial_piv_lu_inverse_u64_c64()\n")
    assert rc == -6, (rc, err)
    assert "libfaer_v0_23_partial_piv_lu_inverse_u64_c64: scalar type not implemented" in err, err


# ---- the yardstick itself: the restatement in the working precision stays inside the backward-error bound on the GPU test's shapes
def gpu_shapes():
    F = fa()
    out = set()
    for dt in (np.complex64, np.complex128):
        w, leaf = F.debug_clu_shape(dt)
        out |= {(1, 1), (2, 2), (3, 3), (31, 31), (33, 33), (w, w), (w + 1, w + 1), (129, 129), (257, 257), (300, 8), (8, 300), (40, 17), (17, 40),
                (leaf, w), (leaf + 1, w), (2000, 64), (5000, 40), (700, 700)}
    return sorted(out)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_the_restatement_is_within_the_backward_error_bound(dtype):
    worst = 0.0
    for m, n in gpu_shapes():
        a = ref.gaussian(m, n, dtype, 7 + m + 3 * n)
        lu, perm, count = ref.lu_unblocked(a)
        assert lu.dtype == np.dtype(dtype)
        e = ref.lu_backward_error(a, lu, perm)
        worst = max(worst, e)
        assert e <= 1.0, (m, n, e)
        rec, moved = ref.records_from_perm(perm, min(m, n))
        assert moved == count
        l, _ = ref.split(lu)
        assert np.abs(np.tril(l, -1)).max(initial=0) <= np.sqrt(2) * (1 + 4 * np.finfo(dtype).eps)
    print(f"{np.dtype(dtype).name}: worst backward error of the restatement {worst:.3f} of the bound")


def test_real_data_takes_the_real_pivots():
    import oracle.oracle as oracle

    for m, n in ((40, 17), (17, 40), (129, 129)):
        a = np.asfortranarray(np.random.default_rng(m + n).standard_normal((m, n)))
        _, perm, count = ref.lu_unblocked(a.astype(np.complex128))
        b = a.copy(order="F")
        operm, _, ocount = oracle.lu_in_place(b)
        assert np.array_equal(perm, operm) and count == ocount, (m, n)


def test_exact_case_is_reproduced_by_the_restatement():
    for n in (40, 130):
        for dtype in (np.complex64, np.complex128):
            a, l, u = ref.exact_case(n, dtype)
            assert np.array_equal(a, (l.astype(np.complex128) @ u.astype(np.complex128)).astype(dtype))
            lu, perm, count = ref.lu_unblocked(a)
            assert count == 0 and np.array_equal(perm, np.arange(n))
            gl, gu = ref.split(lu)
            assert np.array_equal(gl, l) and np.array_equal(gu, u)
