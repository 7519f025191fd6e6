"""CPU tests of the Cholesky update boundary (include/faer_hip.h, "Modifying an existing Cholesky factorization"): every symbol is
declared and exported, the kernel shape and the scratch query answer without a device, and the calls that have nothing to do
return before they touch one (this suite runs on machines without a GPU, where a device touch aborts the process)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_util import fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ([f"faer_hip_llt_rank_r_update_clobber_{s}" for s in ("f64", "f32")]
           + [f"faer_hip_ldlt_rank_r_update_clobber_{s}" for s in ("f64", "f32")]
           + [f"faer_hip_ldlt_delete_rows_and_cols_clobber_{i}_{s}" for i in ("u32", "u64") for s in ("f64", "f32")]
           + [f"faer_hip_ldlt_delete_rows_and_cols_clobber_scratch_{s}" for s in ("f64", "f32")]
           + ["faer_hip_debug_chol_update_last", "faer_hip_debug_chol_update_diag_only", "faer_hip_chol_update_shape"])


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "faer_hip.h")).read()
    L = fa().lib()
    for name in SYMBOLS:
        assert re.search(r"FAER_HIP_API\s+\w+\s+" + name + r"\(", hdr), name
        assert hasattr(L, name), name
    mk = open(os.path.join(ROOT, "faer-rs_amd", "csrc", "Makefile")).read()
    assert "chol_update.hip" in mk
    for f in ("llt_rank_r_update_clobber", "ldlt_rank_r_update_clobber", "ldlt_delete_rows_and_cols_clobber", "debug_chol_update_last",
              "chol_update_shape"):
        assert callable(getattr(fa(), f)), f


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shape_without_device(dtype):
    nb, rc = fa().chol_update_shape(dtype)
    assert nb == 64 and 1 <= rc <= 32


@pytest.mark.parametrize("dtype,isz", [(np.float64, 8), (np.float32, 4)])
def test_scratch_query(dtype, isz):
    F = fa()
    for dim, r in [(300, 7), (1, 1), (0, 0), (16384, 8), (5, 0)]:
        length, align = F.ldlt_delete_rows_and_cols_clobber_scratch(dim, r, dtype)
        assert length == (dim * r + r) * isz and align > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nothing_to_do_returns_without_device(dtype):
    F = fa()
    # n == 0
    l0, w0 = np.zeros((0, 0), dtype=dtype, order="F"), np.zeros((0, 3), dtype=dtype, order="F")
    assert F.llt_rank_r_update_clobber(l0, w0, np.ones(3, dtype=dtype)) is None
    F.ldlt_rank_r_update_clobber(l0, w0, np.ones(3, dtype=dtype))
    # r == 0: L keeps its bits
    l = np.asfortranarray(np.arange(16, dtype=dtype).reshape(4, 4))
    keep = l.copy()
    assert F.llt_rank_r_update_clobber(l, np.zeros((4, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype)) is None
    F.ldlt_rank_r_update_clobber(l, np.zeros((4, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype))
    for it in (np.uint32, np.uint64):
        out = F.ldlt_delete_rows_and_cols_clobber(l, [], index_dtype=it)
        assert out.dtype == it and out.size == 0
    assert np.array_equal(l, keep)
    assert len(F.debug_chol_update_last()) == 4


def test_status_struct_is_the_llt_one():
    F = fa()
    assert C.sizeof(F.LltStatus) == 16 and F.LltStatus.value.offset == 8
