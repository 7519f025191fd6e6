"""CPU tests of the pivoted Cholesky boundary (include/faer_hip.h section 2h): parameter constructor, struct layouts, the scratch
queries without a device, the exported spellings, and -- where the reference header is present -- the layouts against
faer-ffi/faer.h."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_H = os.path.join(os.environ.get("FAER_REFERENCE", "/root/reference"), "faer-ffi", "faer.h")
NAMES = ("piv_llt_factor_in_place_scratch", "piv_llt_factor_in_place", "piv_llt_solve_in_place_scratch", "piv_llt_solve_in_place",
         "piv_llt_reconstruct_scratch", "piv_llt_reconstruct", "piv_llt_inverse_scratch", "piv_llt_inverse")


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_params_constructor(suf):
    F = fa()
    p = getattr(F.lib(), f"libfaer_v0_23_PivLltParams_{suf}")()
    assert p.block_size == 128


def test_struct_sizes_and_tags():
    F = fa()
    assert C.sizeof(F.PivLltParams) == 8 and F.PivLltParams.block_size.offset == 0
    assert C.sizeof(F.PivLltStatus) == 24 and F.PivLltStatus.rank.offset == 8 and F.PivLltStatus.transposition_count.offset == 16
    assert (F.PIV_LLT_OK, F.PIV_LLT_NON_POSITIVE_PIVOT, F.PIV_LLT_UNKNOWN) == (0, 1, 2)
    st = F.PivLltStatus(1, 5, 0)
    assert st.index == 5  # non_positive_pivot.index shares the union with ok.rank


@pytest.mark.parametrize("it", ["u32", "u64"])
@pytest.mark.parametrize("suf,isz", [("f64", 8), ("f32", 4)])
def test_scratch_queries_without_device(it, suf, isz):
    F = fa()
    L = F.lib()
    p = getattr(L, f"libfaer_v0_23_PivLltParams_{suf}")()
    fac = getattr(L, f"libfaer_v0_23_piv_llt_factor_in_place_scratch_{it}_{suf}")
    sol = getattr(L, f"libfaer_v0_23_piv_llt_solve_in_place_scratch_{it}_{suf}")
    rec = getattr(L, f"libfaer_v0_23_piv_llt_reconstruct_scratch_{it}_{suf}")
    inv = getattr(L, f"libfaer_v0_23_piv_llt_inverse_scratch_{it}_{suf}")
    lay = fac(C.c_size_t(300), F.PAR_SEQ, p)
    assert lay.len_bytes >= 2 * 300 * isz and lay.align_bytes > 0  # factor.rs:37-45: two columns of real scalars
    assert sol(C.c_size_t(300), C.c_size_t(7), F.PAR_SEQ).len_bytes >= 300 * 7 * isz  # solve.rs:4-11
    assert rec(C.c_size_t(300), F.PAR_SEQ).len_bytes >= 300 * 300 * isz  # reconstruct.rs:4-10
    assert inv(C.c_size_t(300), F.PAR_SEQ).len_bytes >= 300 * 300 * isz  # inverse.rs:4-10
    for lay in (fac(C.c_size_t(0), F.PAR_SEQ, p), sol(C.c_size_t(0), C.c_size_t(3), F.PAR_SEQ), rec(C.c_size_t(0), F.PAR_SEQ),
                inv(C.c_size_t(0), F.PAR_SEQ)):
        assert lay.len_bytes == 0 and lay.align_bytes > 0


def test_spellings_exported():
    L = fa().lib()
    for v in ("v0_23", "v0_24"):
        for suf in ("f64", "f32"):
            assert hasattr(L, f"libfaer_{v}_PivLltParams_{suf}")
            for it in ("u32", "u64"):
                for name in NAMES:
                    assert hasattr(L, f"libfaer_{v}_{name}_{it}_{suf}"), (v, name, it, suf)
        for suf in ("fx128", "c32", "c64", "cx128"):  # the aborting stubs of the scalar types that are not implemented
            assert hasattr(L, f"libfaer_{v}_PivLltParams_{suf}")
            assert hasattr(L, f"libfaer_{v}_piv_llt_factor_in_place_u64_{suf}")
    assert hasattr(L, "faer_hip_debug_piv_llt_last")
    assert len(fa().debug_piv_llt_last()) == 4


def test_layouts_against_reference_header(tmp_path):
    if not os.path.exists(REF_H):
        pytest.skip("reference faer.h not available")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "piv_llt_layout.c"
    src.write_text(f"""
#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>
#include "{REF_H}"
#define FAER_HIP_NO_FFI_PROTOTYPES
#include "{os.path.join(ROOT, 'include', 'faer_hip.h')}"
_Static_assert(sizeof(FaerPivLltParams) == sizeof(FaerV0_24_PivLltParams), "params size");
_Static_assert(offsetof(FaerPivLltParams, block_size) == offsetof(FaerV0_24_PivLltParams, block_size), "block_size");
_Static_assert(sizeof(FaerPivLltStatus) == sizeof(FaerV0_24_PivLltStatus), "status size");
_Static_assert(offsetof(FaerPivLltStatus, tag) == offsetof(FaerV0_24_PivLltStatus, tag), "status tag");
_Static_assert(offsetof(FaerPivLltStatus, ok) == offsetof(FaerV0_24_PivLltStatus, ok), "status union");
_Static_assert(offsetof(FaerPivLltStatus, ok.rank) == offsetof(FaerV0_24_PivLltStatus, ok.rank), "rank");
_Static_assert(offsetof(FaerPivLltStatus, ok.transposition_count) == offsetof(FaerV0_24_PivLltStatus, ok.transposition_count), "count");
_Static_assert(offsetof(FaerPivLltStatus, non_positive_pivot.index) == offsetof(FaerV0_24_PivLltStatus, non_positive_pivot.index), "index");
_Static_assert((int) FaerPivLltStatus_Ok == (int) FaerV0_24_PivLltStatus_Ok, "tag values");
_Static_assert((int) FaerPivLltStatus_NonPositivePivot == (int) FaerV0_24_PivLltStatus_NonPositivePivot, "tag values");
_Static_assert((int) FaerPivLltStatus_Unknown == (int) FaerV0_24_PivLltStatus_Unknown, "tag values");
int main(void) {{ return 0; }}
""")
    subprocess.check_call([cc, "-std=c11", "-c", str(src), "-o", str(tmp_path / "piv_llt_layout.o")])
