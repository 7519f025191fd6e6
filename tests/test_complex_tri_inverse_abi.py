"""CPU tests of the complex triangular-inverse boundary (include/faer_hip.h: inverse_{,unit_}triangular_{lower,upper}_in_place for
c32 / c64): the prototypes are declared with the f64 argument lists, both spellings are exported and resolve to one address, the
dimension check that precedes any staging aborts with its own message (in a child process), a real-only family stays a stub -- and
the yardstick of tests/test_gpu_complex_tri_inverse.py is reachable by the plain numpy restatement on the inputs that file uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import complex_tri_inverse_ref as ref
from complex_cases import C_TRI_COMPLEX, ceps
from gpu_util import fa
from test_complex_abi import child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("inverse_triangular_lower_in_place", "inverse_triangular_upper_in_place", "inverse_unit_triangular_lower_in_place",
         "inverse_unit_triangular_upper_in_place")
NAMES = [f"libfaer_v0_23_{f}_{s}" for f in FORMS for s in ("c32", "c64")]


def test_header_declares_the_prototypes_with_the_f64_argument_lists():
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    assert len(NAMES) == 8
    for name in NAMES:
        decl = re.search(r"FAER_HIP_API\s+(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        decl64 = re.search(r"FAER_HIP_API\s+(\w+)\s+" + name[:-3] + r"f64\(([^;]*)\);", hdr)
        assert decl and decl64, name
        assert decl.groups() == decl64.groups(), name
    assert re.search(r"FAER_HIP_API\s+void\s+faer_hip_debug_ctrtri_shape\(int elem_bytes, size_t out\[2\]\);", hdr)


def test_both_spellings_are_exported_and_are_one_function():
    F = fa()
    out = subprocess.run(["nm", "-D", "--defined-only", F.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert "faer_hip_debug_ctrtri_shape" in exported
    dl = C.CDLL(None)
    dl.dlsym.restype = C.c_void_p
    dl.dlsym.argtypes = [C.c_void_p, C.c_char_p]
    handle = C.c_void_p(F.lib()._handle)
    for name in NAMES:
        new = name.replace("v0_23", "v0_24")
        assert name in exported and new in exported, name
        # an empty call returns at once, needs no device, and leaves the jump's PLT slot bound whatever the binding mode
        z = np.zeros((0, 0), np.complex64 if name.endswith("c32") else np.complex128, order="F")
        getattr(F.lib(), new)(F._mat(z, F.MatMut), F._mat(z), F.PAR_SEQ)
        a, b = dl.dlsym(handle, name.encode()), dl.dlsym(handle, new.encode())
        assert a and b, name
        # the v0_24 spelling is a tail jump (csrc/abi_compat.c): one `jmp rel32` through the PLT to the v0_23 entry, nothing else
        code = C.string_at(b, 5)
        assert code[0] == 0xE9, (name, code.hex())
        assert resolve_jump(b) == a, name


def resolve_jump(addr):
    """follows `jmp rel32` and the PLT's `[endbr64;] [bnd] jmp *disp(%rip)` from addr to the function it lands in"""
    for _ in range(4):
        code = C.string_at(addr, 16)
        if code[:4] == b"\xf3\x0f\x1e\xfa":  # endbr64
            addr += 4
            continue
        if code[0] == 0xE9:
            addr = addr + 5 + int.from_bytes(code[1:5], "little", signed=True)
            continue
        off = 1 if code[0] == 0xF2 else 0  # bnd prefix
        if code[off:off + 2] == b"\xff\x25":
            slot = addr + off + 6 + int.from_bytes(code[off + 2:off + 6], "little", signed=True)
            return C.c_void_p.from_address(slot).value
        return addr
    return addr


def test_shape_query():
    F = fa()
    for dt in (np.complex64, np.complex128):
        e, sub = F.debug_ctrtri_shape(dt)
        assert e >= 16 and sub >= 1 and e % sub == 0 and (e // sub) % 16 == 0
        assert 2 * e * e * np.dtype(dt).itemsize <= 160 * 1024  # the block and as much again for padding and the intermediate fit the LDS
    assert F.debug_ctrtri_shape(np.complex64)[0] >= F.debug_ctrtri_shape(np.complex128)[0]


def test_inverse_c64_lower_checks_dimensions_before_anything_else():
    rc, err = child("t = np.eye(3, dtype=np.complex128, order='F'); w = np.zeros((4, 4), np.complex128, order='F')\n"
                    "F.inverse_triangular_in_place(w, t, upper=False, unit=False)\nprint('returned')\n")
    assert rc == -6, (rc, err)
    assert "triangular inverse: dimension mismatch" in err and "scalar type not implemented" not in err, err


def test_inverse_c32_unit_upper_checks_dimensions_before_anything_else():
    rc, err = child("t = np.eye(3, dtype=np.complex64, order='F'); w = np.zeros((3, 2), np.complex64, order='F')\n"
                    "F.inverse_triangular_in_place(w, t, upper=True, unit=True)\nprint('returned')\n")
    assert rc == -6, (rc, err)
    assert "triangular inverse: dimension mismatch" in err and "scalar type not implemented" not in err, err


def test_real_only_family_still_ends_in_its_stub():
    rc, err = child("F.lib().libfaer_v0_23_llt_factor_in_place_c64()\n")
    assert rc == -6, (rc, err)
    assert "libfaer_v0_23_llt_factor_in_place_c64: scalar type not implemented" in err, err


# ---- the yardstick itself: the restatement in the working precision has a small residual on every input of the GPU test
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_the_restatement_meets_the_residual_bound(dtype):
    """C_TRI_COMPLEX n eps, the componentwise bound of the complex triangular solves (complex_cases.py), holds for both residuals of the
    restatement: the GPU test's yardstick FACTOR * max(r_ref, eps) is therefore a small multiple of the format's precision"""
    F = fa()
    worst = 0.0
    for n in ref.sizes(*F.debug_ctrtri_shape(dtype)):
        for triangle, unit in ref.VARIANTS:
            t, tp, w, r = ref.case(n, dtype, triangle, unit)
            assert w.dtype == np.dtype(dtype) and np.isfinite(w).all()
            assert np.isnan(tp[~ref.written_mask(n, triangle, unit)]).all()
            q = r / (C_TRI_COMPLEX * n * ceps(dtype))
            worst = max(worst, q)
            assert q <= 1.0, (n, triangle, unit, r)
    print(f"{np.dtype(dtype).name}: worst residual of the restatement {worst:.3f} of the bound")


def test_exact_case_is_reproduced_by_the_restatement():
    for dtype in (np.complex64, np.complex128):
        e = fa().debug_ctrtri_shape(dtype)[0]
        for n in (e + 1, 3 * e + 5):
            for triangle, unit in ref.VARIANTS:
                t, w = ref.exact_case(n, dtype, triangle, unit)
                assert np.array_equal(ref.recursive_inverse(t, triangle, unit), w), (n, triangle, unit)
                assert ref.residual(t, w, triangle, unit) == 0.0


def test_sentinel_is_a_nan_with_its_payload():
    for dt in (np.complex64, np.complex128):
        s = ref.sentinel(5, dt)
        assert s.flags.f_contiguous and np.isnan(s.real).all() and np.isnan(s.imag).all()
        assert ref.same_bits(s, ref.sentinel(5, dt)) and not ref.same_bits(s, np.full((5, 5), np.nan + 1j * np.nan, dtype=dt, order="F"))
