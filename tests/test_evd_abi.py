"""CPU tests of the self-adjoint EVD boundary (include/faer_hip.h section 2e): parameter constructors, struct layouts,
the scratch query, and -- where the reference header is present -- the layouts against faer-ffi/faer.h."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_H = os.path.join(os.environ.get("FAER_REFERENCE", "/root/reference"), "faer-ffi", "faer.h")


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_params_constructors(suf):
    F = fa()
    L = F.lib()
    f = getattr(L, f"libfaer_v0_23_SelfAdjointEvdParams_{suf}")
    f.restype = F.SelfAdjointEvdParams
    p = f()
    assert (p.tridiag.par_threshold, p.recursion_threshold) == (192 * 256, 128)
    g = getattr(L, f"libfaer_v0_23_TridiagParams_{suf}")
    g.restype = F.TridiagParams
    assert g().par_threshold == 192 * 256


def test_struct_sizes():
    F = fa()
    assert C.sizeof(F.EvdStatus) == 16
    assert C.sizeof(F.SelfAdjointEvdParams) == 16
    assert C.sizeof(F.TridiagParams) == 8


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_scratch_query_without_device(suf):
    F = fa()
    L = F.lib()
    p = getattr(L, f"libfaer_v0_23_SelfAdjointEvdParams_{suf}")
    p.restype = F.SelfAdjointEvdParams
    fn = getattr(L, f"libfaer_v0_23_self_adjoint_evd_scratch_{suf}")
    fn.restype = F.Layout
    for compute_u in (0, 1):
        lay = fn(C.c_size_t(100), C.c_int(compute_u), F.PAR_SEQ, p())
        assert lay.len_bytes > 0 and lay.align_bytes > 0


def test_v0_24_spellings_exported():
    L = fa().lib()
    for name in ("self_adjoint_evd", "self_adjoint_evd_scratch", "SelfAdjointEvdParams", "TridiagParams"):
        for v in ("v0_23", "v0_24"):
            for suf in ("f64", "f32"):
                assert hasattr(L, f"libfaer_{v}_{name}_{suf}")


def test_layouts_against_reference_header(tmp_path):
    if not os.path.exists(REF_H):
        pytest.skip("reference faer.h not available")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "evd_layout.c"
    src.write_text(f"""
#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>
#include "{REF_H}"
#define FAER_HIP_NO_FFI_PROTOTYPES
#include "{os.path.join(ROOT, 'include', 'faer_hip.h')}"
_Static_assert(sizeof(FaerEvdStatus) == sizeof(FaerV0_24_EvdStatus), "EvdStatus size");
_Static_assert(offsetof(FaerEvdStatus, tag) == offsetof(FaerV0_24_EvdStatus, tag), "EvdStatus tag");
_Static_assert(offsetof(FaerEvdStatus, ok) == offsetof(FaerV0_24_EvdStatus, ok), "EvdStatus union");
_Static_assert(sizeof(FaerSelfAdjointEvdParams) == sizeof(FaerV0_24_SelfAdjointEvdParams), "params size");
_Static_assert(offsetof(FaerSelfAdjointEvdParams, tridiag) == offsetof(FaerV0_24_SelfAdjointEvdParams, tridiag), "tridiag");
_Static_assert(offsetof(FaerSelfAdjointEvdParams, recursion_threshold) == offsetof(FaerV0_24_SelfAdjointEvdParams, recursion_threshold), "rt");
_Static_assert(sizeof(FaerTridiagParams) == sizeof(FaerV0_24_TridiagParams), "TridiagParams");
_Static_assert((int) FaerEvdStatus_NoConvergence == (int) FaerV0_24_EvdStatus_NoConvergence, "tag values");
_Static_assert((int) FaerComputeEigenvectors_Yes == (int) FaerV0_24_ComputeEigenvectors_Yes, "ComputeEigenvectors");
int main(void) {{ return 0; }}
""")
    subprocess.check_call([cc, "-std=c11", "-c", str(src), "-o", str(tmp_path / "evd_layout.o")])
