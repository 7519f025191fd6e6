"""CPU tests of the SVD boundary (include/faer_hip.h section 2f): parameter constructors, struct layouts, the scratch
query, and -- where the reference header is present -- the layouts against faer-ffi/faer.h."""
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
    f = getattr(L, f"libfaer_v0_23_SvdParams_{suf}")
    f.restype = F.SvdParams
    p = f()
    q = getattr(L, f"libfaer_v0_23_QrParams_{suf}")
    q.restype = F.QrParams
    qd = q()
    assert p.bidiag.par_threshold == 192 * 256
    assert (p.qr.blocking_threshold, p.qr.par_threshold) == (qd.blocking_threshold, qd.par_threshold)
    assert p.recursion_threshold == 128
    assert p.qr_ratio_threshold == 11.0 / 6.0
    g = getattr(L, f"libfaer_v0_23_BidiagParams_{suf}")
    g.restype = F.BidiagParams
    assert g().par_threshold == 192 * 256


def test_struct_sizes():
    F = fa()
    assert C.sizeof(F.SvdStatus) == 16
    assert C.sizeof(F.SvdParams) == 40
    assert C.sizeof(F.BidiagParams) == 8
    assert (F.SVD_OK, F.SVD_NO_CONVERGENCE) == (0, 1)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_scratch_query_without_device(suf):
    F = fa()
    L = F.lib()
    p = getattr(L, f"libfaer_v0_23_SvdParams_{suf}")
    p.restype = F.SvdParams
    fn = getattr(L, f"libfaer_v0_23_svd_scratch_{suf}")
    fn.restype = F.Layout
    for compute_u in (0, 1, 2):
        for compute_v in (0, 1, 2):
            for m, n in ((300, 100), (100, 300)):
                lay = fn(C.c_size_t(m), C.c_size_t(n), C.c_int(compute_u), C.c_int(compute_v), F.PAR_SEQ, p())
                assert lay.len_bytes > 0 and lay.align_bytes > 0
            lay = fn(C.c_size_t(0), C.c_size_t(5), C.c_int(compute_u), C.c_int(compute_v), F.PAR_SEQ, p())
            assert lay.len_bytes == 0 and lay.align_bytes > 0


def test_v0_24_spellings_exported():
    L = fa().lib()
    for name in ("svd", "svd_scratch", "SvdParams", "BidiagParams"):
        for v in ("v0_23", "v0_24"):
            for suf in ("f64", "f32"):
                assert hasattr(L, f"libfaer_{v}_{name}_{suf}")


def test_layouts_against_reference_header(tmp_path):
    if not os.path.exists(REF_H):
        pytest.skip("reference faer.h not available")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "svd_layout.c"
    src.write_text(f"""
#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>
#include "{REF_H}"
#define FAER_HIP_NO_FFI_PROTOTYPES
#include "{os.path.join(ROOT, 'include', 'faer_hip.h')}"
_Static_assert(sizeof(FaerSvdStatus) == sizeof(FaerV0_24_SvdStatus), "SvdStatus size");
_Static_assert(offsetof(FaerSvdStatus, tag) == offsetof(FaerV0_24_SvdStatus, tag), "SvdStatus tag");
_Static_assert(offsetof(FaerSvdStatus, ok) == offsetof(FaerV0_24_SvdStatus, ok), "SvdStatus union");
_Static_assert(sizeof(FaerSvdParams) == sizeof(FaerV0_24_SvdParams), "params size");
_Static_assert(offsetof(FaerSvdParams, bidiag) == offsetof(FaerV0_24_SvdParams, bidiag), "bidiag");
_Static_assert(offsetof(FaerSvdParams, qr) == offsetof(FaerV0_24_SvdParams, qr), "qr");
_Static_assert(offsetof(FaerSvdParams, recursion_threshold) == offsetof(FaerV0_24_SvdParams, recursion_threshold), "rt");
_Static_assert(offsetof(FaerSvdParams, qr_ratio_threshold) == offsetof(FaerV0_24_SvdParams, qr_ratio_threshold), "ratio");
_Static_assert(sizeof(FaerBidiagParams) == sizeof(FaerV0_24_BidiagParams), "BidiagParams");
_Static_assert((int) FaerSvdStatus_Ok == (int) FaerV0_24_SvdStatus_Ok, "tag values");
_Static_assert((int) FaerSvdStatus_NoConvergence == (int) FaerV0_24_SvdStatus_NoConvergence, "tag values");
_Static_assert((int) FaerComputeSvdVectors_No == (int) FaerV0_24_ComputeSvdVectors_No, "ComputeSvdVectors");
_Static_assert((int) FaerComputeSvdVectors_Thin == (int) FaerV0_24_ComputeSvdVectors_Thin, "ComputeSvdVectors");
_Static_assert((int) FaerComputeSvdVectors_Full == (int) FaerV0_24_ComputeSvdVectors_Full, "ComputeSvdVectors");
int main(void) {{ return 0; }}
""")
    subprocess.check_call([cc, "-std=c11", "-c", str(src), "-o", str(tmp_path / "svd_layout.o")])
