"""CPU-side checks of the generalized EVD boundary: both dtypes and both spellings of every symbol, the struct layouts of faer.h,
the defaults of the *Params constructors, and the scratch query (answered without a GPU, monotone in dim).  No compute calls."""
import ctypes as C

import pytest

from gpu_util import fa

NAMES = ["generalized_evd", "generalized_evd_scratch", "GeneralizedHessenbergParams", "GeneralizedSchurParams", "GevdParams"]


@pytest.mark.parametrize("ver", ["v0_23", "v0_24"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_symbols_exist(ver, suf):
    lib = fa().lib()
    for name in NAMES:
        assert hasattr(lib, f"libfaer_{ver}_{name}_{suf}"), name
    for other in ("c32", "c64", "fx128", "cx128"):  # aborting stubs, so that the reference's C++ wrapper links
        assert hasattr(lib, f"libfaer_{ver}_generalized_evd_{other}")


def test_struct_layouts_match_faer_h():
    F = fa()
    w = C.sizeof(C.c_size_t)
    assert C.sizeof(F.GeneralizedHessenbergParams) == 2 * w
    assert [f[0] for f in F.GeneralizedHessenbergParams._fields_] == ["block_size", "blocking_threshold"]
    assert C.sizeof(F.GeneralizedSchurParams) == 5 * w
    assert [f[0] for f in F.GeneralizedSchurParams._fields_] == ["relative_cost_estimate_of_shift_chase_to_matmul", "recommended_shift_count",
                                                                 "recommended_deflation_window", "blocking_threshold", "nibble_threshold"]
    assert F.GeneralizedSchurParams.blocking_threshold.offset == 3 * w and F.GeneralizedSchurParams.nibble_threshold.offset == 4 * w
    assert C.sizeof(F.GevdFromSchurParams) == w
    assert C.sizeof(F.GevdParams) == 8 * w
    assert (F.GevdParams.hessenberg.offset, F.GevdParams.schur.offset, F.GevdParams.evd_from_schur.offset) == (0, 2 * w, 7 * w)
    assert C.sizeof(F.GevdStatus) == 2 * w and F.GevdStatus.padding.offset == w
    assert (F.GEVD_OK, F.GEVD_NO_CONVERGENCE) == (0, 1)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_defaults(suf):
    F = fa()
    lib = F.lib()
    f = getattr(lib, f"libfaer_v0_23_GeneralizedHessenbergParams_{suf}")
    f.restype = F.GeneralizedHessenbergParams
    p = f()
    assert (p.block_size, p.blocking_threshold) == (32, 256 * 256)
    f = getattr(lib, f"libfaer_v0_23_GeneralizedSchurParams_{suf}")
    f.restype = F.GeneralizedSchurParams
    s = f()
    g = getattr(lib, f"libfaer_v0_23_SchurParams_{suf}")
    g.restype = F.SchurParams
    e = g()
    assert s.relative_cost_estimate_of_shift_chase_to_matmul(100, 50) == 10 and s.relative_cost_estimate_of_shift_chase_to_matmul(5000, 7) == 10
    for n in (10, 100, 1000, 10000):
        assert s.recommended_shift_count(n, n) == e.recommended_shift_count(n, n) == lib.faer_hip_default_recommended_shift_count(C.c_size_t(n), C.c_size_t(n))
        assert s.recommended_deflation_window(n, n) == e.recommended_deflation_window(n, n)
    assert (s.blocking_threshold, s.nibble_threshold) == (e.blocking_threshold, e.nibble_threshold)
    f = getattr(lib, f"libfaer_v0_24_GevdParams_{suf}")
    f.restype = F.GevdParams
    p = f()
    assert (p.hessenberg.block_size, p.hessenberg.blocking_threshold, p.schur.nibble_threshold) == (32, 256 * 256, e.nibble_threshold)
    assert p.schur.relative_cost_estimate_of_shift_chase_to_matmul(1, 1) == 10


@pytest.mark.parametrize("suf,isz", [("f64", 8), ("f32", 4)])
def test_scratch_query_needs_no_gpu_and_is_monotone(suf, isz):
    F = fa()
    lib = F.lib()
    pf = getattr(lib, f"libfaer_v0_23_GevdParams_{suf}")
    pf.restype = F.GevdParams
    q = getattr(lib, f"libfaer_v0_23_generalized_evd_scratch_{suf}")
    q.restype = F.Layout
    assert q(C.c_size_t(0), 1, 1, F.PAR_SEQ, pf()).len_bytes == 0
    for left, right in ((0, 0), (1, 0), (0, 1), (1, 1)):
        prev = 0
        for dim in (1, 2, 3, 63, 64, 65, 96, 97, 131, 197, 293, 1024):
            lay = q(C.c_size_t(dim), left, right, F.PAR_SEQ, pf())
            assert lay.len_bytes >= prev and lay.len_bytes >= 2 * dim * dim * isz
            prev = lay.len_bytes
    assert q(C.c_size_t(100), 1, 1, F.PAR_SEQ, pf()).len_bytes > q(C.c_size_t(100), 0, 0, F.PAR_SEQ, pf()).len_bytes
    assert F.gevd_window_edge("float64") == 64 and F.gevd_window_edge("float32") == 96
