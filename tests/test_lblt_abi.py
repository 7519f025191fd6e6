"""CPU tests of the LBLT boundary (include/faer_hip.h section 2g): parameter constructor, struct layouts, the scratch queries
without a device, the exported spellings, and -- where the reference header is present -- the layouts against faer-ffi/faer.h."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_H = os.path.join(os.environ.get("FAER_REFERENCE", "/root/reference"), "faer-ffi", "faer.h")
NAMES = ("lblt_factor_in_place_scratch", "lblt_factor_in_place", "lblt_solve_in_place_scratch", "lblt_solve_in_place",
         "lblt_reconstruct_scratch", "lblt_reconstruct", "lblt_inverse_scratch", "lblt_inverse")


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_params_constructor(suf):
    F = fa()
    p = getattr(F.lib(), f"libfaer_v0_23_LbltParams_{suf}")()
    assert (p.pivoting, p.par_threshold, p.block_size) == (F.PIVOTING_PARTIAL_DIAG, 128 * 128, 64)


def test_struct_sizes_and_enum():
    F = fa()
    assert C.sizeof(F.LbltParams) == 24 and F.LbltParams.par_threshold.offset == 8 and F.LbltParams.block_size.offset == 16
    assert C.sizeof(F.LbltStatus) == 16 and F.LbltStatus.transposition_count.offset == 8
    assert (F.PIVOTING_PARTIAL, F.PIVOTING_PARTIAL_DIAG, F.PIVOTING_ROOK, F.PIVOTING_ROOK_DIAG, F.PIVOTING_FULL) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("it", ["u32", "u64"])
@pytest.mark.parametrize("suf,isz", [("f64", 8), ("f32", 4)])
def test_scratch_queries_without_device(it, suf, isz):
    F = fa()
    L = F.lib()
    p = getattr(L, f"libfaer_v0_23_LbltParams_{suf}")()
    fac = getattr(L, f"libfaer_v0_23_lblt_factor_in_place_scratch_{it}_{suf}")
    sol = getattr(L, f"libfaer_v0_23_lblt_solve_in_place_scratch_{it}_{suf}")
    rec = getattr(L, f"libfaer_v0_23_lblt_reconstruct_scratch_{it}_{suf}")
    inv = getattr(L, f"libfaer_v0_23_lblt_inverse_scratch_{it}_{suf}")
    # factor.rs:1128-1140: dim indices, plus a dim x block_size panel only above the block size
    small, big = fac(C.c_size_t(64), F.PAR_SEQ, p), fac(C.c_size_t(300), F.PAR_SEQ, p)
    assert 64 * 8 <= small.len_bytes < 64 * 8 + 64
    assert big.len_bytes >= 300 * 8 + 300 * 64 * isz and big.align_bytes > 0
    assert sol(C.c_size_t(300), C.c_size_t(7), F.PAR_SEQ).len_bytes >= 300 * 7 * isz  # solve.rs:11-18
    assert rec(C.c_size_t(300), F.PAR_SEQ).len_bytes >= 300 * 300 * isz  # reconstruct.rs:4-10
    assert inv(C.c_size_t(300), F.PAR_SEQ).len_bytes >= 300 * 300 * isz  # inverse.rs:3-9
    for lay in (fac(C.c_size_t(0), F.PAR_SEQ, p), sol(C.c_size_t(0), C.c_size_t(3), F.PAR_SEQ), rec(C.c_size_t(0), F.PAR_SEQ),
                inv(C.c_size_t(0), F.PAR_SEQ)):
        assert lay.len_bytes == 0 and lay.align_bytes > 0


def test_spellings_exported():
    L = fa().lib()
    for v in ("v0_23", "v0_24"):
        for suf in ("f64", "f32"):
            assert hasattr(L, f"libfaer_{v}_LbltParams_{suf}")
            for it in ("u32", "u64"):
                for name in NAMES:
                    assert hasattr(L, f"libfaer_{v}_{name}_{it}_{suf}"), (v, name, it, suf)
    assert hasattr(L, "faer_hip_debug_lblt_last")
    assert fa().debug_lblt_last() == (0, 0, 0, 0) or len(fa().debug_lblt_last()) == 4


def test_layouts_against_reference_header(tmp_path):
    if not os.path.exists(REF_H):
        pytest.skip("reference faer.h not available")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "lblt_layout.c"
    src.write_text(f"""
#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>
#include "{REF_H}"
#define FAER_HIP_NO_FFI_PROTOTYPES
#include "{os.path.join(ROOT, 'include', 'faer_hip.h')}"
_Static_assert(sizeof(FaerLbltParams) == sizeof(FaerV0_24_LbltParams), "params size");
_Static_assert(offsetof(FaerLbltParams, pivoting) == offsetof(FaerV0_24_LbltParams, pivoting), "pivoting");
_Static_assert(offsetof(FaerLbltParams, par_threshold) == offsetof(FaerV0_24_LbltParams, par_threshold), "par_threshold");
_Static_assert(offsetof(FaerLbltParams, block_size) == offsetof(FaerV0_24_LbltParams, block_size), "block_size");
_Static_assert(sizeof(FaerLbltStatus) == sizeof(FaerV0_24_LbltStatus), "status size");
_Static_assert(offsetof(FaerLbltStatus, tag) == offsetof(FaerV0_24_LbltStatus, tag), "status tag");
_Static_assert(offsetof(FaerLbltStatus, ok) == offsetof(FaerV0_24_LbltStatus, ok), "status union");
_Static_assert((int) FaerLbltStatus_Ok == (int) FaerV0_24_LbltStatus_Ok, "tag values");
_Static_assert((int) FaerLbltStatus_Unknown == (int) FaerV0_24_LbltStatus_Unknown, "tag values");
_Static_assert((int) FaerPivotingStrategy_Partial == (int) FaerV0_24_PivotingStrategy_Partial, "strategy");
_Static_assert((int) FaerPivotingStrategy_PartialDiag == (int) FaerV0_24_PivotingStrategy_PartialDiag, "strategy");
_Static_assert((int) FaerPivotingStrategy_Rook == (int) FaerV0_24_PivotingStrategy_Rook, "strategy");
_Static_assert((int) FaerPivotingStrategy_RookDiag == (int) FaerV0_24_PivotingStrategy_RookDiag, "strategy");
_Static_assert((int) FaerPivotingStrategy_Full == (int) FaerV0_24_PivotingStrategy_Full, "strategy");
_Static_assert(sizeof(FaerPivotingStrategy) == sizeof(FaerV0_24_PivotingStrategy), "enum size");
int main(void) {{ return 0; }}
""")
    subprocess.check_call([cc, "-std=c11", "-c", str(src), "-o", str(tmp_path / "lblt_layout.o")])
