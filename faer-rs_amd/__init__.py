"""faer_rs_amd -- thin host-side mirror of faer's low-level API over libfaer_hip.so.

Everything here is plumbing: it builds the repr(C) structs of include/faer_hip.h from numpy arrays
(host memory) or torch tensors (device memory) and calls the C-ABI through ctypes.  The compute lives in
the shared library (hand-written HIP for gfx950); there is no Python or CPU compute path, and importing
`lib()` raises if the library has not been built (run `python -c "import __graft_entry__ as g; g.build()"`).

Function names, argument order and error behaviour follow the reference:
  matmul                      faer/src/linalg/matmul/mod.rs:1617
  matmul_triangular           faer/src/linalg/matmul/triangular.rs:1193
  solve_*_triangular_in_place faer/src/linalg/triangular_solve.rs:220-419
  llt_factor_in_place         faer/src/linalg/cholesky/llt/factor.rs:67   (Result<LltInfo, LltError>)
  partial_piv_lu_factor_in_place  faer/src/linalg/lu/partial_pivoting/factor.rs:234
  qr_factor_in_place          faer/src/linalg/qr/no_pivoting/factor.rs:258
  Llt / PartialPivLu / Qr     faer/src/linalg/solvers.rs:770-1204 (high level owners)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfaer_hip.so")
if os.environ.get("FAER_HIP_LIB"):  # developer override (instrumented builds); never a different backend
    LIB_PATH = os.environ["FAER_HIP_LIB"]
_LIB = None

# ------------------------------------------------------------------ repr(C) structs (include/faer_hip.h)


class MatRef(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("nrows", C.c_size_t), ("ncols", C.c_size_t), ("row_stride", C.c_ssize_t),
                ("col_stride", C.c_ssize_t)]


class MatMut(MatRef):
    pass


class SliceMut(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_size_t)]


class SliceRef(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_size_t)]


class Par(C.Structure):
    _fields_ = [("tag", C.c_int), ("nthreads", C.c_size_t)]


class Layout(C.Structure):
    _fields_ = [("len_bytes", C.c_size_t), ("align_bytes", C.c_size_t)]


class MemAlloc(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len_bytes", C.c_size_t)]


class LltStatus(C.Structure):
    _fields_ = [("tag", C.c_int), ("value", C.c_size_t)]


class PartialPivLuStatus(C.Structure):
    _fields_ = [("tag", C.c_int), ("transposition_count", C.c_size_t)]


class QrStatus(C.Structure):
    _fields_ = [("tag", C.c_int), ("rank", C.c_size_t)]


class LltParams(C.Structure):
    _fields_ = [("recursion_threshold", C.c_size_t), ("block_size", C.c_size_t)]


class PartialPivLuParams(C.Structure):
    _fields_ = [("recursion_threshold", C.c_size_t), ("block_size", C.c_size_t), ("par_threshold", C.c_size_t)]


class QrParams(C.Structure):
    _fields_ = [("blocking_threshold", C.c_size_t), ("par_threshold", C.c_size_t)]


class LdltRegularization(C.Structure):
    """include/faer_hip.h FaerLdltRegularization {delta*, epsilon*, signs: SliceMut of i8}"""
    _fields_ = [("dynamic_regularization_delta", C.c_void_p), ("dynamic_regularization_epsilon", C.c_void_p),
                ("dynamic_regularization_signs", SliceMut)]


class VecRef(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("len", C.c_size_t), ("stride", C.c_ssize_t)]


class VecMut(VecRef):
    pass


class LbltParams(C.Structure):
    """include/faer_hip.h FaerLbltParams {pivoting, par_threshold, block_size} (the ffi order)"""
    _fields_ = [("pivoting", C.c_int), ("par_threshold", C.c_size_t), ("block_size", C.c_size_t)]


class LbltStatus(C.Structure):
    """include/faer_hip.h FaerLbltStatus: tag (0 Ok, 1 Unknown), then ok.transposition_count"""
    _fields_ = [("tag", C.c_int), ("transposition_count", C.c_size_t)]


class PivLltParams(C.Structure):
    """include/faer_hip.h FaerPivLltParams {block_size}"""
    _fields_ = [("block_size", C.c_size_t)]


class PivLltStatus(C.Structure):
    """include/faer_hip.h FaerPivLltStatus: tag (0 Ok, 1 NonPositivePivot, 2 Unknown), then the union of ok {rank, transposition_count}
    and non_positive_pivot {index} (`rank` doubles as the index)"""
    _fields_ = [("tag", C.c_int), ("rank", C.c_size_t), ("transposition_count", C.c_size_t)]

    @property
    def index(self):
        return self.rank


PIV_LLT_OK, PIV_LLT_NON_POSITIVE_PIVOT, PIV_LLT_UNKNOWN = 0, 1, 2


# include/faer_hip.h FaerPivotingStrategy
PIVOTING_PARTIAL, PIVOTING_PARTIAL_DIAG, PIVOTING_ROOK, PIVOTING_ROOK_DIAG, PIVOTING_FULL = 0, 1, 2, 3, 4
PivotingStrategy = {"partial": 0, "partial_diag": 1, "rook": 2, "rook_diag": 3, "full": 4}


class LdltError(Exception):
    """faer::linalg::cholesky::ldlt::factor::LdltError::ZeroPivot { index }"""

    def __init__(self, index):
        super().__init__(f"ZeroPivot {{ index: {index} }}")
        self.index = index


class LltRegularization(C.Structure):
    _fields_ = [("dynamic_regularization_delta", C.c_void_p), ("dynamic_regularization_epsilon", C.c_void_p)]


class TridiagParams(C.Structure):
    _fields_ = [("par_threshold", C.c_size_t)]


class SelfAdjointEvdParams(C.Structure):
    """include/faer_hip.h FaerSelfAdjointEvdParams {tridiag: {par_threshold}, recursion_threshold}"""
    _fields_ = [("tridiag", TridiagParams), ("recursion_threshold", C.c_size_t)]


class EvdStatus(C.Structure):
    """include/faer_hip.h FaerEvdStatus: tag (0 Ok, 1 NoConvergence), then a union of one size_t"""
    _fields_ = [("tag", C.c_int), ("padding", C.c_size_t)]


EVD_OK, EVD_NO_CONVERGENCE = 0, 1

SHIFT_FN = C.CFUNCTYPE(C.c_size_t, C.c_size_t, C.c_size_t)


class HessenbergParams(C.Structure):
    _fields_ = [("par_threshold", C.c_size_t), ("blocking_threshold", C.c_size_t)]


class SchurParams(C.Structure):
    """include/faer_hip.h FaerSchurParams: two function pointers (matrix dimension, active block dimension) -> size_t, two sizes"""
    _fields_ = [("recommended_shift_count", SHIFT_FN), ("recommended_deflation_window", SHIFT_FN),
                ("blocking_threshold", C.c_size_t), ("nibble_threshold", C.c_size_t)]


class EvdFromSchurParams(C.Structure):
    _fields_ = [("recursion_threshold", C.c_size_t)]


class EvdParams(C.Structure):
    """include/faer_hip.h FaerEvdParams {hessenberg, schur, evd_from_schur}"""
    _fields_ = [("hessenberg", HessenbergParams), ("schur", SchurParams), ("evd_from_schur", EvdFromSchurParams)]


class GeneralizedHessenbergParams(C.Structure):
    _fields_ = [("block_size", C.c_size_t), ("blocking_threshold", C.c_size_t)]


class GeneralizedSchurParams(C.Structure):
    """include/faer_hip.h FaerGeneralizedSchurParams: three function pointers (matrix dimension, active block dimension) -> size_t, two sizes"""
    _fields_ = [("relative_cost_estimate_of_shift_chase_to_matmul", SHIFT_FN), ("recommended_shift_count", SHIFT_FN),
                ("recommended_deflation_window", SHIFT_FN), ("blocking_threshold", C.c_size_t), ("nibble_threshold", C.c_size_t)]


class GevdFromSchurParams(C.Structure):
    _fields_ = [("padding", C.c_size_t)]


class GevdParams(C.Structure):
    """include/faer_hip.h FaerGevdParams {hessenberg, schur, evd_from_schur}"""
    _fields_ = [("hessenberg", GeneralizedHessenbergParams), ("schur", GeneralizedSchurParams), ("evd_from_schur", GevdFromSchurParams)]


class GevdStatus(C.Structure):
    """include/faer_hip.h FaerGevdStatus: tag (0 Ok, 1 NoConvergence), then a union of one size_t"""
    _fields_ = [("tag", C.c_int), ("padding", C.c_size_t)]


GEVD_OK, GEVD_NO_CONVERGENCE = 0, 1


class BidiagParams(C.Structure):
    _fields_ = [("par_threshold", C.c_size_t)]


class SvdParams(C.Structure):
    """include/faer_hip.h FaerSvdParams {bidiag: {par_threshold}, qr: {blocking_threshold, par_threshold},
    recursion_threshold, qr_ratio_threshold}"""
    _fields_ = [("bidiag", BidiagParams), ("qr", QrParams), ("recursion_threshold", C.c_size_t),
                ("qr_ratio_threshold", C.c_double)]


class SvdStatus(C.Structure):
    """include/faer_hip.h FaerSvdStatus: tag (0 Ok, 1 NoConvergence), then a union of one size_t"""
    _fields_ = [("tag", C.c_int), ("padding", C.c_size_t)]


SVD_OK, SVD_NO_CONVERGENCE = 0, 1


BCAST_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)


class Comm(C.Structure):
    _fields_ = [("rank", C.c_int), ("world_size", C.c_int), ("bcast", BCAST_FN), ("user", C.c_void_p)]


ACCUM_REPLACE, ACCUM_ADD = 0, 1
CONJ_NO, CONJ_YES = 0, 1
BLOCK = {"rect": 0, "lower": 1, "upper": 2, "strict_lower": 3, "strict_upper": 4, "unit_lower": 5, "unit_upper": 6}
DST_FULL, DST_LOWER, DST_UPPER = 0, 1, 2
DTYPE_F32, DTYPE_F64, DTYPE_C32, DTYPE_C64 = 0, 1, 2, 3
PAR_SEQ = Par(0, 1)


class LltError(Exception):
    """faer::linalg::cholesky::llt::factor::LltError::NonPositivePivot { index }"""

    def __init__(self, index):
        super().__init__(f"NonPositivePivot {{ index: {index} }}")
        self.index = index


def lib():
    """Loads libfaer_hip.so.  Fails loudly when it is missing: there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc, gfx950). "
                           "faer_rs_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for suf in ("f64", "f32"):
        getattr(L, f"libfaer_v0_23_llt_factor_in_place_{suf}").restype = LltStatus
        getattr(L, f"libfaer_v0_23_qr_factor_in_place_{suf}").restype = QrStatus
        getattr(L, f"libfaer_v0_23_qr_recommended_block_size_{suf}").restype = C.c_size_t
        getattr(L, f"libfaer_v0_23_LltParams_{suf}").restype = LltParams
        getattr(L, f"libfaer_v0_23_LdltParams_{suf}").restype = LltParams
        getattr(L, f"libfaer_v0_23_ldlt_factor_in_place_{suf}").restype = LltStatus
        getattr(L, f"libfaer_v0_23_ldlt_factor_in_place_scratch_{suf}").restype = Layout
        getattr(L, f"libfaer_v0_23_ldlt_solve_in_place_scratch_{suf}").restype = Layout
        getattr(L, f"libfaer_v0_23_PartialPivLuParams_{suf}").restype = PartialPivLuParams
        getattr(L, f"libfaer_v0_23_QrParams_{suf}").restype = QrParams
        for it in ("u32", "u64"):
            getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_{it}_{suf}").restype = PartialPivLuStatus
            getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_{it}_{suf}").restype = Layout
        for name in ("llt_factor_in_place_scratch", "llt_solve_in_place_scratch", "qr_factor_in_place_scratch",
                     "apply_householder_on_the_left_scratch", "apply_householder_transpose_on_the_left_scratch"):
            getattr(L, f"libfaer_v0_23_{name}_{suf}").restype = Layout
        getattr(L, f"faer_hip_dist_partial_piv_lu_{suf}").restype = PartialPivLuStatus
        getattr(L, f"libfaer_v0_23_LbltParams_{suf}").restype = LbltParams
        for it in ("u32", "u64"):
            getattr(L, f"libfaer_v0_23_lblt_factor_in_place_{it}_{suf}").restype = LbltStatus
            for name in ("lblt_factor_in_place_scratch", "lblt_solve_in_place_scratch", "lblt_reconstruct_scratch", "lblt_inverse_scratch"):
                getattr(L, f"libfaer_v0_23_{name}_{it}_{suf}").restype = Layout
        getattr(L, f"libfaer_v0_23_PivLltParams_{suf}").restype = PivLltParams
        for it in ("u32", "u64"):
            getattr(L, f"libfaer_v0_23_piv_llt_factor_in_place_{it}_{suf}").restype = PivLltStatus
            for name in ("piv_llt_factor_in_place_scratch", "piv_llt_solve_in_place_scratch", "piv_llt_reconstruct_scratch",
                         "piv_llt_inverse_scratch"):
                getattr(L, f"libfaer_v0_23_{name}_{it}_{suf}").restype = Layout
    for suf in ("c64", "c32"):  # complex partial-pivot LU
        getattr(L, f"libfaer_v0_23_PartialPivLuParams_{suf}").restype = PartialPivLuParams
        for it in ("u32", "u64"):
            getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_{it}_{suf}").restype = PartialPivLuStatus
            for name in ("partial_piv_lu_factor_in_place_scratch", "partial_piv_lu_solve_in_place_scratch",
                         "partial_piv_lu_solve_transpose_in_place_scratch"):
                getattr(L, f"libfaer_v0_23_{name}_{it}_{suf}").restype = Layout
    L.libfaer_v0_23_get_global_par.restype = Par
    L.faer_hip_version.restype = C.c_char_p
    L.faer_hip_device_count.restype = C.c_int
    L.faer_hip_lblt_pivoting_supported.restype = C.c_int
    L.faer_hip_get_stream.restype = C.c_void_p
    L.faer_hip_malloc.restype = C.c_void_p
    L.faer_hip_time_gemm_ms.restype = C.c_double
    L.faer_hip_mfma_peak_tflops.restype = C.c_double
    if hasattr(L, "faer_hip_xwg_hop_us"):  # (absent from older builds loaded through FAER_HIP_LIB for A/B runs)
        L.faer_hip_xwg_hop_us.restype = C.c_double
    L.faer_hip_dist_local_ncols.restype = C.c_size_t
    L.faer_hip_dist_panel_ws_scalars.restype = C.c_size_t
    _LIB = L
    import atexit

    atexit.register(L.faer_hip_shutdown)
    return L


# ------------------------------------------------------------------ operand marshalling
def _is_torch(x):
    return type(x).__module__.startswith("torch")


class C32(C.Structure):
    """faer's c32: repr(C) {re, im}; built from any Python / numpy scalar"""
    _fields_ = [("re", C.c_float), ("im", C.c_float)]

    def __init__(self, z=0):
        z = complex(z)
        super().__init__(z.real, z.imag)


class C64(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]

    def __init__(self, z=0):
        z = complex(z)
        super().__init__(z.real, z.imag)


def _dtype_suffix(x):
    """(suffix of the entry points, ctypes constructor of one scalar, bytes per element); complex scalars exist at level 3 and in the
    partial-pivot LU only"""
    if _is_torch(x):
        import torch

        if x.dtype == torch.float64:
            return "f64", C.c_double, 8
        if x.dtype == torch.float32:
            return "f32", C.c_float, 4
        if x.dtype == torch.complex128:
            return "c64", C64, 16
        if x.dtype == torch.complex64:
            return "c32", C32, 8
    else:
        if x.dtype == np.float64:
            return "f64", C.c_double, 8
        if x.dtype == np.float32:
            return "f32", C.c_float, 4
        if x.dtype == np.complex128:
            return "c64", C64, 16
        if x.dtype == np.complex64:
            return "c32", C32, 8
    raise TypeError(f"faer_rs_amd supports f32 / f64 (and c32 / c64 in matmul, matmul_triangular, gemm, the triangular solves and inverses and the "
                    f"partial-pivot LU with its solves), got {x.dtype}")


def _mat(x, cls=MatRef):
    """2-D numpy array / torch tensor -> MatRef/MatMut (strides in elements)."""
    if _is_torch(x):
        assert x.dim() == 2
        return cls(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x.stride(1))
    assert x.ndim == 2
    it = x.itemsize
    return cls(x.ctypes.data, x.shape[0], x.shape[1], x.strides[0] // it, x.strides[1] // it)


def use_torch_stream():
    """Enqueue on torch's current HIP stream (torch is plumbing here: memory + streams)."""
    import torch

    lib().faer_hip_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))


def synchronize():
    lib().faer_hip_synchronize()


# ------------------------------------------------------------------ low level API (faer::linalg)
def matmul(c, accum, a, b, alpha=1.0, par=PAR_SEQ):
    suf, ct, _ = _dtype_suffix(c)
    al = ct(alpha)
    getattr(lib(), f"libfaer_v0_23_matmul_{suf}")(_mat(c, MatMut), C.c_int(accum), _mat(a), _mat(b), C.byref(al), par)
    return c


def matmul_triangular(c, c_block, accum, a, a_block, b, b_block, alpha=1.0, par=PAR_SEQ):
    suf, ct, _ = _dtype_suffix(c)
    al = ct(alpha)
    getattr(lib(), f"libfaer_v0_23_matmul_triangular_{suf}")(_mat(c, MatMut), C.c_int(BLOCK[c_block]), C.c_int(accum),
                                                           _mat(a), C.c_int(BLOCK[a_block]), _mat(b),
                                                           C.c_int(BLOCK[b_block]), C.byref(al), par)
    return c


def gemm(dst, dst_kind, accum, lhs, rhs, alpha=1.0, row_idx=None, col_idx=None, diag=None, conj_lhs=False, conj_rhs=False):
    """inner boundary: the private_gemm_x86::gemm call of faer (include/faer_hip.h section 1).  conj_lhs / conj_rhs conjugate a
    complex operand (the identity for real ones); complex products take no row_idx / col_idx / diag."""
    suf, ct, _ = _dtype_suffix(dst)
    al = ct(alpha)
    m, k = lhs.shape
    n = rhs.shape[1]
    d = _mat(dst, MatMut)
    a, b = _mat(lhs), _mat(rhs)

    def idx(v):
        if v is None:
            return None, 1
        if _is_torch(v):  # device index array: int32 / int64 storage read as u32 / u64 (indices are non-negative)
            import torch

            assert v.dtype in (torch.int32, torch.int64) and v.is_contiguous()
            return C.c_void_p(v.data_ptr()), (1 if v.dtype == torch.int64 else 0)
        assert v.dtype in (np.uint32, np.uint64)
        return C.c_void_p(v.ctypes.data), (1 if v.dtype == np.uint64 else 0)

    ri, it1 = idx(row_idx)
    ci, it2 = idx(col_idx)
    itype = it1 if row_idx is not None else it2
    dg, dgs = (None, 0)
    if diag is not None:
        dg = C.c_void_p(diag.data_ptr() if _is_torch(diag) else diag.ctypes.data)
        dgs = diag.stride(0) if _is_torch(diag) else diag.strides[0] // diag.itemsize
    lib().faer_hip_gemm(C.c_int({"f32": DTYPE_F32, "f64": DTYPE_F64, "c32": DTYPE_C32, "c64": DTYPE_C64}[suf]), C.c_int(itype), C.c_size_t(m), C.c_size_t(n),
                        C.c_size_t(k), C.c_void_p(d.ptr), C.c_ssize_t(d.row_stride), C.c_ssize_t(d.col_stride), ri, ci,
                        C.c_int(dst_kind), C.c_int(accum), C.c_void_p(a.ptr), C.c_ssize_t(a.row_stride),
                        C.c_ssize_t(a.col_stride), C.c_bool(bool(conj_lhs)), dg, C.c_ssize_t(dgs), C.c_void_p(b.ptr),
                        C.c_ssize_t(b.row_stride), C.c_ssize_t(b.col_stride), C.c_bool(bool(conj_rhs)), C.byref(al), C.c_size_t(0))
    return dst


GEMM_PLAN_INPUTS = ("m", "n", "k", "elem_bytes", "kind", "add", "alpha_sign", "drs", "dcs", "ars", "acs", "brs", "bcs", "indexed", "diag",
                    "a_struct", "b_struct", "k_trim", "tri_skip", "stair_nb", "stair_gap", "stair_row0", "prefer_big_tiles", "variant")
GEMM_PLAN_FIELDS = ("transposed", "tile", "tri_skip_split", "akm", "bkm", "bm", "bn", "ntm", "ntn", "tri_enum", "tri_off", "splits",
                    "k_per_split", "fast_io", "prof_class", "routes")
GEMM_TILES = ("Extra64", "Pipe64", "Pipe128", "PipeWide", "Legacy64", "Legacy128")


def debug_gemm_plan(**problem):
    """faer_hip_debug_gemm_plan (no GPU needed): the dense dispatch's plan for a product given as GEMM_PLAN_INPUTS (m, n, k and
    elem_bytes are required, strides default to column-major operands, everything else to 0) -> dict of GEMM_PLAN_FIELDS, or the
    refusal message as a str, or None if it is not a dense product"""
    q = dict(drs=1, dcs=problem["m"], ars=1, acs=problem["m"], brs=1, bcs=problem["k"])
    q.update(problem)
    assert set(q) <= set(GEMM_PLAN_INPUTS), set(q) - set(GEMM_PLAN_INPUTS)
    inp = (C.c_longlong * len(GEMM_PLAN_INPUTS))(*(int(q.get(f, 0)) for f in GEMM_PLAN_INPUTS))
    out = (C.c_int * len(GEMM_PLAN_FIELDS))()
    why = C.c_char_p()
    rc = lib().faer_hip_debug_gemm_plan(inp, out, C.byref(why))
    if rc == 0:
        return dict(zip(GEMM_PLAN_FIELDS, out))
    return why.value.decode() if rc == 1 else None


def _trsm(name, t, rhs, par, conj=False):
    """rhs <- op(t)^-1 rhs; conj: op is the conjugate (complex scalars; the real entry points ignore it)"""
    suf, _, _ = _dtype_suffix(rhs)
    getattr(lib(), f"libfaer_v0_23_{name}_{suf}")(_mat(t), C.c_int(CONJ_YES if conj else CONJ_NO), _mat(rhs, MatMut), par)
    return rhs


def solve_lower_triangular_in_place(l, rhs, par=PAR_SEQ, conj=False):
    return _trsm("solve_triangular_lower_in_place", l, rhs, par, conj)


def solve_upper_triangular_in_place(u, rhs, par=PAR_SEQ, conj=False):
    return _trsm("solve_triangular_upper_in_place", u, rhs, par, conj)


def solve_unit_lower_triangular_in_place(l, rhs, par=PAR_SEQ, conj=False):
    return _trsm("solve_unit_triangular_lower_in_place", l, rhs, par, conj)


def solve_unit_upper_triangular_in_place(u, rhs, par=PAR_SEQ, conj=False):
    return _trsm("solve_unit_triangular_upper_in_place", u, rhs, par, conj)


def llt_factor_in_place(a, regularization=(0.0, 0.0), par=PAR_SEQ):
    """returns dynamic_regularization_count; raises LltError(index) like Err(NonPositivePivot{index})"""
    suf, ct, _ = _dtype_suffix(a)
    delta, eps = ct(regularization[0]), ct(regularization[1])
    reg = LltRegularization(C.cast(C.pointer(delta), C.c_void_p), C.cast(C.pointer(eps), C.c_void_p))
    L = lib()
    params = getattr(L, f"libfaer_v0_23_LltParams_{suf}")()
    st = getattr(L, f"libfaer_v0_23_llt_factor_in_place_{suf}")(_mat(a, MatMut), reg, par, MemAlloc(None, 0), params)
    if st.tag == 0:
        return st.value
    if st.tag == 1:
        raise LltError(st.value)
    raise RuntimeError("LltStatus::Unknown")


def ldlt_factor_in_place(a, regularization=(0.0, 0.0), signs=None, par=PAR_SEQ):
    """cholesky/ldlt/factor.rs:742-800: unit lower L strictly below the diagonal of `a`, D on it.
    returns dynamic_regularization_count; raises LdltError(index) like Err(ZeroPivot{index})"""
    suf, ct, _ = _dtype_suffix(a)
    delta, eps = ct(regularization[0]), ct(regularization[1])
    sl = SliceMut(None, 0)
    if signs is not None:
        signs = np.ascontiguousarray(signs, dtype=np.int8)
        sl = SliceMut(signs.ctypes.data, signs.shape[0])
    reg = LdltRegularization(C.cast(C.pointer(delta), C.c_void_p), C.cast(C.pointer(eps), C.c_void_p), sl)
    L = lib()
    params = getattr(L, f"libfaer_v0_23_LdltParams_{suf}")()
    st = getattr(L, f"libfaer_v0_23_ldlt_factor_in_place_{suf}")(_mat(a, MatMut), reg, par, MemAlloc(None, 0), params)
    if st.tag == 0:
        return st.value
    if st.tag == 1:
        raise LdltError(st.value)
    raise RuntimeError("LdltStatus::Unknown")


def ldlt_solve_in_place(ld, rhs, par=PAR_SEQ):
    """cholesky/ldlt/solve.rs:12-50 with L and D packed as ldlt_factor_in_place leaves them"""
    suf, _, _ = _dtype_suffix(ld)
    n = ld.shape[0]
    if _is_torch(ld):
        d = VecRef(ld.data_ptr(), n, ld.stride(0) + ld.stride(1))
    else:
        d = VecRef(ld.ctypes.data, n, (ld.strides[0] + ld.strides[1]) // ld.itemsize)
    getattr(lib(), f"libfaer_v0_23_ldlt_solve_in_place_{suf}")(_mat(ld), d, C.c_int(0), _mat(rhs, MatMut), par, MemAlloc(None, 0))
    return rhs


def llt_solve_in_place(l, rhs, par=PAR_SEQ):
    suf, _, _ = _dtype_suffix(rhs)
    getattr(lib(), f"libfaer_v0_23_llt_solve_in_place_{suf}")(_mat(l), C.c_int(CONJ_NO), _mat(rhs, MatMut), par,
                                                            MemAlloc(None, 0))
    return rhs


def partial_piv_lu_factor_in_place(a, index_dtype=np.uint64, par=PAR_SEQ):
    """returns (perm_fwd, perm_bwd, transposition_count); perm_fwd[i] = source row of row i of P*A"""
    suf, _, _ = _dtype_suffix(a)
    m = a.shape[0]
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    fwd = np.zeros(m, dtype=index_dtype)
    bwd = np.zeros(m, dtype=index_dtype)
    L = lib()
    params = getattr(L, f"libfaer_v0_23_PartialPivLuParams_{suf}")()
    st = getattr(L, f"libfaer_v0_23_partial_piv_lu_factor_in_place_{it}_{suf}")(
        _mat(a, MatMut), SliceMut(fwd.ctypes.data, m), SliceMut(bwd.ctypes.data, m), par, MemAlloc(None, 0), params)
    if st.tag != 0:
        raise RuntimeError("PartialPivLuStatus::Unknown")
    return fwd, bwd, st.transposition_count


class FullPivLuParams(C.Structure):
    _fields_ = [("par_threshold", C.c_size_t)]


def full_piv_lu_factor_in_place(a, index_dtype=np.uint64, par=PAR_SEQ):
    """lu/full_pivoting/factor.rs:452-525.  returns (row_fwd, row_bwd, col_fwd, col_bwd, transposition_count):
    A[row_fwd][:, col_fwd] == L U with L unit lower trapezoidal and U upper trapezoidal packed in `a`"""
    suf, _, _ = _dtype_suffix(a)
    m, n = a.shape
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    rf, rb = np.zeros(m, dtype=index_dtype), np.zeros(m, dtype=index_dtype)
    cf, cb = np.zeros(n, dtype=index_dtype), np.zeros(n, dtype=index_dtype)
    L = lib()
    pf = getattr(L, f"libfaer_v0_23_FullPivLuParams_{suf}")
    pf.restype = FullPivLuParams
    fn = getattr(L, f"libfaer_v0_23_full_piv_lu_factor_in_place_{it}_{suf}")
    fn.restype = PartialPivLuStatus  # same layout: {tag, transposition_count}
    st = fn(_mat(a, MatMut), SliceMut(rf.ctypes.data, m), SliceMut(rb.ctypes.data, m), SliceMut(cf.ctypes.data, n), SliceMut(cb.ctypes.data, n),
            par, MemAlloc(None, 0), pf())
    if st.tag != 0:
        raise RuntimeError("FullPivLuStatus::Unknown")
    return rf, rb, cf, cb, st.transposition_count


def full_piv_lu_solve_in_place(lu, row_fwd, row_bwd, col_fwd, col_bwd, rhs, transpose=False, par=PAR_SEQ):
    """lu/full_pivoting/solve.rs: rhs <- A^-1 rhs (or A^-T rhs)"""
    suf, _, _ = _dtype_suffix(lu)
    it = "u64" if np.dtype(row_fwd.dtype) == np.uint64 else "u32"
    name = "full_piv_lu_solve_transpose_in_place" if transpose else "full_piv_lu_solve_in_place"
    n = lu.shape[0]
    getattr(lib(), f"libfaer_v0_23_{name}_{it}_{suf}")(
        _mat(lu), _mat(lu), C.c_int(0), SliceRef(row_fwd.ctypes.data, n), SliceRef(row_bwd.ctypes.data, n), SliceRef(col_fwd.ctypes.data, n),
        SliceRef(col_bwd.ctypes.data, n), _mat(rhs, MatMut), par, MemAlloc(None, 0))
    return rhs


class ColPivQrParams(C.Structure):
    _fields_ = [("blocking_threshold", C.c_size_t), ("par_threshold", C.c_size_t)]


def colpiv_qr_factor_in_place(a, q_coeff, index_dtype=np.uint64, par=PAR_SEQ):
    """qr/col_pivoting/factor.rs:356-395.  returns (col_fwd, col_bwd, transposition_count): A[:, col_fwd] == Q R with the
    Householder basis below the diagonal of `a`, R on and above it, block factors in q_coeff (block_size x min(m, n))"""
    suf, _, _ = _dtype_suffix(a)
    n = a.shape[1]
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    cf, cb = np.zeros(n, dtype=index_dtype), np.zeros(n, dtype=index_dtype)
    L = lib()
    pf = getattr(L, f"libfaer_v0_23_ColPivQrParams_{suf}")
    pf.restype = ColPivQrParams
    fn = getattr(L, f"libfaer_v0_23_colpiv_qr_factor_in_place_{it}_{suf}")
    fn.restype = PartialPivLuStatus  # same layout: {tag, transposition_count}
    st = fn(_mat(a, MatMut), _mat(q_coeff, MatMut), SliceMut(cf.ctypes.data, n), SliceMut(cb.ctypes.data, n), par, MemAlloc(None, 0), pf())
    if st.tag != 0:
        raise RuntimeError("ColPivQrStatus::Unknown")
    return cf, cb, st.transposition_count


def tridiag_in_place(a, householder):
    """faer::linalg::evd::tridiag::tridiag_in_place (evd/tridiag.rs:274): `a` (n x n, self-adjoint, only the lower triangle
    is used) -> the tridiagonal T on its diagonal / subdiagonal (a = Q T Q^H), the reflectors of Q below the subdiagonal,
    their block factors in `householder` (block_size x (n - 1))"""
    suf, _, _ = _dtype_suffix(a)
    fn = getattr(lib(), f"faer_hip_tridiag_in_place_{suf}")
    fn.restype = None
    fn(_mat(a, MatMut), _mat(householder, MatMut))
    return a, householder


def self_adjoint_evd(a, s, u=None, params=None, par=PAR_SEQ):
    """faer::linalg::evd::self_adjoint_evd (evd/mod.rs:270): eigenvalues of the self-adjoint `a` (n x n, only its lower
    triangle is read, never written) in ascending order into the 1-D `s`; with `u` (n x n) the orthonormal eigenvectors,
    column j going with s[j].  Returns the status tag (EVD_OK or EVD_NO_CONVERGENCE)."""
    suf, _, _ = _dtype_suffix(a)
    L = lib()
    if params is None:
        pf = getattr(L, f"libfaer_v0_23_SelfAdjointEvdParams_{suf}")
        pf.restype = SelfAdjointEvdParams
        params = pf()
    if _is_torch(s):
        assert s.dim() == 1
        sv = VecRef(s.data_ptr(), s.shape[0], s.stride(0))
    else:
        assert s.ndim == 1
        sv = VecRef(s.ctypes.data, s.shape[0], s.strides[0] // s.itemsize)
    um = _mat(u, MatMut) if u is not None else MatMut(None, a.shape[0], 0, 1, a.shape[0])
    fn = getattr(L, f"libfaer_v0_23_self_adjoint_evd_{suf}")
    fn.restype = EvdStatus
    st = fn(_mat(a), um, sv, par, MemAlloc(None, 0), params)
    return st.tag


def evd(a, s, s_im, ul=None, ur=None, params=None, par=PAR_SEQ):
    """faer::linalg::evd::evd_real (evd/mod.rs:1213): eigenvalues of the general real `a` (n x n, never written), real parts
    into the 1-D `s`, imaginary parts into `s_im`; with `ul` / `ur` (n x n) the left / right eigenvectors in the reference's
    packed layout (a real eigenvalue: column i; a pair at (i, i + 1): real part, imaginary part).  Returns the status tag
    (EVD_OK or EVD_NO_CONVERGENCE)."""
    suf, _, _ = _dtype_suffix(a)
    L = lib()
    if params is None:
        pf = getattr(L, f"libfaer_v0_23_EvdParams_{suf}")
        pf.restype = EvdParams
        params = pf()
    n = a.shape[0]
    ulm = _mat(ul, MatMut) if ul is not None else MatMut(None, n, 0, 1, n)
    urm = _mat(ur, MatMut) if ur is not None else MatMut(None, n, 0, 1, n)
    fn = getattr(L, f"libfaer_v0_23_evd_{suf}")
    fn.restype = EvdStatus
    st = fn(_mat(a), ulm, urm, _vec(s, VecMut), _vec(s_im, VecMut), par, MemAlloc(None, 0), params)
    return st.tag


def debug_evd_last_counts():
    """{sweeps, window steps, leaf launches, state read-backs} of the calling thread's last evd"""
    out = (C.c_long * 4)()
    lib().faer_hip_debug_evd_last_counts(out)
    return dict(zip(("sweeps", "window_steps", "leaves", "readbacks"), (int(v) for v in out)))


def evd_window_edge(dtype):
    """W: the edge of the LDS-resident window of the Schur kernels (96 for float64, 128 for float32)"""
    f = lib().faer_hip_evd_window_edge
    f.restype = C.c_size_t
    return int(f(C.c_int(DTYPE_F64 if np.dtype(dtype) == np.float64 else DTYPE_F32)))


def generalized_evd(a, b, alpha, alpha_im, beta, ul=None, ur=None, params=None, par=PAR_SEQ):
    """faer::linalg::gevd::gevd_real (gevd/mod.rs:130): eigenvalues (alpha + i alpha_im) / beta of the real pair (`a`, `b`) (n x n,
    never written) into the 1-D `alpha`, `alpha_im`, `beta`; with `ul` / `ur` (n x n) the left / right eigenvectors in the packed
    layout of evd.  Returns the status tag (GEVD_OK or GEVD_NO_CONVERGENCE)."""
    suf, _, _ = _dtype_suffix(a)
    L = lib()
    if params is None:
        pf = getattr(L, f"libfaer_v0_23_GevdParams_{suf}")
        pf.restype = GevdParams
        params = pf()
    n = a.shape[0]
    ulm = _mat(ul, MatMut) if ul is not None else MatMut(None, n, 0, 1, n)
    urm = _mat(ur, MatMut) if ur is not None else MatMut(None, n, 0, 1, n)
    fn = getattr(L, f"libfaer_v0_23_generalized_evd_{suf}")
    fn.restype = GevdStatus
    st = fn(_mat(a, MatMut), _mat(b, MatMut), ulm, urm, _vec(alpha, VecMut), _vec(alpha_im, VecMut), _vec(beta, VecMut), par, MemAlloc(None, 0), params)
    return st.tag


def debug_gevd_last_counts():
    """{multishift sweeps, window steps, leaf launches, state read-backs, infinite eigenvalues deflated} of the calling thread's last generalized_evd"""
    out = (C.c_long * 5)()
    lib().faer_hip_debug_gevd_last_counts(out)
    return dict(zip(("sweeps", "window_steps", "leaves", "readbacks", "infinite_deflations"), (int(v) for v in out)))


def gevd_window_edge(dtype):
    """W: the edge of the LDS-resident leaf and window of the QZ kernels (64 for float64, 96 for float32)"""
    f = lib().faer_hip_gevd_window_edge
    f.restype = C.c_size_t
    return int(f(C.c_int(DTYPE_F64 if np.dtype(dtype) == np.float64 else DTYPE_F32)))


def llt_rank_r_update_clobber(l, w, alpha, raise_on_error=True):
    """faer::linalg::cholesky::llt::update::rank_r_update_clobber (llt/update.rs:360): the factor in the lower triangle of `l` (n x n)
    becomes that of A + w diag(alpha) w^T (`w` n x r, `alpha` 1-D with r entries; a negative alpha downdates).  `w` and `alpha` are
    clobbered.  Each operand is a numpy array or a device tensor on its own.  Raises LltError(index) like Err(NonPositivePivot{index});
    with raise_on_error=False returns the index instead (None: Ok)."""
    suf, _, _ = _dtype_suffix(l)
    fn = getattr(lib(), f"faer_hip_llt_rank_r_update_clobber_{suf}")
    fn.restype = LltStatus
    st = fn(_mat(l, MatMut), _mat(w, MatMut), _vec(alpha, VecMut))
    if st.tag == 0:
        return None
    if st.tag != 1:
        raise RuntimeError("LltStatus::Unknown")
    if raise_on_error:
        raise LltError(st.value)
    return int(st.value)


def ldlt_rank_r_update_clobber(ld, w, alpha):
    """faer::linalg::cholesky::ldlt::update::rank_r_update_clobber (ldlt/update.rs:376): the same for L D L^T packed as
    ldlt_factor_in_place leaves it (unit lower L strictly below the diagonal of `ld`, D on it)"""
    suf, _, _ = _dtype_suffix(ld)
    fn = getattr(lib(), f"faer_hip_ldlt_rank_r_update_clobber_{suf}")
    fn.restype = None
    fn(_mat(ld, MatMut), _mat(w, MatMut), _vec(alpha, VecMut))
    return ld


def ldlt_delete_rows_and_cols_clobber(ld, indices, index_dtype=np.uint64):
    """faer::linalg::cholesky::ldlt::update::delete_rows_and_cols_clobber (ldlt/update.rs:417): the leading (n - r)^2 block of `ld`
    receives the factors of A without the rows and columns `indices`; the trailing r rows are unspecified.  Returns the indices as
    the call left them: sorted, in an array of `index_dtype`."""
    suf, _, _ = _dtype_suffix(ld)
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    idx = np.array(indices, dtype=np.uint64 if it == "u64" else np.uint32).ravel()
    fn = getattr(lib(), f"faer_hip_ldlt_delete_rows_and_cols_clobber_{it}_{suf}")
    fn.restype = None
    fn(_mat(ld, MatMut), SliceMut(idx.ctypes.data if idx.size else None, idx.shape[0]), PAR_SEQ, MemAlloc(None, 0))
    return idx


def ldlt_delete_rows_and_cols_clobber_scratch(dim, n_removed, dtype=np.float64):
    """(len_bytes, align_bytes) of the reference's scratch figure: dim * n_removed + n_removed scalars"""
    fn = getattr(lib(), f"faer_hip_ldlt_delete_rows_and_cols_clobber_scratch_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")
    fn.restype = Layout
    lay = fn(C.c_size_t(dim), C.c_size_t(n_removed))
    return int(lay.len_bytes), int(lay.align_bytes)


def debug_chol_update_last():
    """{column blocks, tail launches, chunks of W per block, host synchronisations inside the block loop} of the calling thread's last
    Cholesky update or deletion"""
    out = (C.c_long * 4)()
    lib().faer_hip_debug_chol_update_last(out)
    return dict(zip(("blocks", "tail_launches", "chunks", "loop_syncs"), (int(v) for v in out)))


def debug_chol_update_diag_only(on):
    """measurement aid: True = only the diagonal kernels of the Cholesky update run (its serial chain; the factor is wrong)"""
    lib().faer_hip_debug_chol_update_diag_only(C.c_int(1 if on else 0))


def chol_update_shape(dtype):
    """(NB, RC): columns per block and columns of W per chunk of the Cholesky update kernels.  Needs no GPU."""
    out = (C.c_size_t * 2)()
    lib().faer_hip_chol_update_shape(C.c_int(DTYPE_F64 if np.dtype(dtype) == np.float64 else DTYPE_F32), out)
    return int(out[0]), int(out[1])


def svd(a, s, u=None, v=None, params=None, par=PAR_SEQ):
    """faer::linalg::svd::svd (svd/mod.rs:530): singular values of `a` (m x n, never written) in nonincreasing order into
    the 1-D `s` (min(m, n) entries); with `u` (m x min(m, n) or m x m) / `v` (n x min(m, n) or n x n) the left / right
    singular vectors, a = u[:, :k] diag(s) v[:, :k]^T.  Returns the status tag (SVD_OK or SVD_NO_CONVERGENCE)."""
    suf, _, _ = _dtype_suffix(a)
    L = lib()
    if params is None:
        pf = getattr(L, f"libfaer_v0_23_SvdParams_{suf}")
        pf.restype = SvdParams
        params = pf()
    if _is_torch(s):
        assert s.dim() == 1
        sv = VecRef(s.data_ptr(), s.shape[0], s.stride(0))
    else:
        assert s.ndim == 1
        sv = VecRef(s.ctypes.data, s.shape[0], s.strides[0] // s.itemsize)
    um = _mat(u, MatMut) if u is not None else MatMut(None, a.shape[0], 0, 1, a.shape[0])
    vm = _mat(v, MatMut) if v is not None else MatMut(None, a.shape[1], 0, 1, a.shape[1])
    fn = getattr(L, f"libfaer_v0_23_svd_{suf}")
    fn.restype = SvdStatus
    st = fn(_mat(a), um, sv, vm, par, MemAlloc(None, 0), params)
    return st.tag


def hessenberg_in_place(a, householder):
    """faer::linalg::evd::hessenberg::hessenberg_in_place (evd/hessenberg.rs:549): `a` (n x n) -> the upper Hessenberg H on and
    above its subdiagonal (a = Q H Q^H), the reflectors of Q below it, their block factors in `householder`
    (block_size x (n - 1))"""
    suf, _, _ = _dtype_suffix(a)
    fn = getattr(lib(), f"faer_hip_hessenberg_in_place_{suf}")
    fn.restype = None
    fn(_mat(a, MatMut), _mat(householder, MatMut))
    return a, householder


def bidiag_in_place(a, h_left, h_right):
    """faer::linalg::svd::bidiag::bidiag_in_place (svd/bidiag.rs:47): `a` -> the upper bidiagonal B on its diagonal /
    superdiagonal (a = U B V^H for nrows >= ncols, the shape the reference's SVD uses), left reflectors below the diagonal
    (block factors h_left: bl x min(m, n)), right reflectors right of the superdiagonal (h_right: br x (min(m, n) - 1))"""
    suf, _, _ = _dtype_suffix(a)
    fn = getattr(lib(), f"faer_hip_bidiag_in_place_{suf}")
    fn.restype = None
    fn(_mat(a, MatMut), _mat(h_left, MatMut), _mat(h_right, MatMut))
    return a, h_left, h_right


def colpiv_qr_solve_in_place(qr, q_coeff, col_fwd, col_bwd, rhs, mode="lstsq", par=PAR_SEQ):
    """qr/col_pivoting/solve.rs; mode: 'lstsq' (m >= n, solution in the first n rows), 'solve' (square), 'transpose'"""
    suf, _, _ = _dtype_suffix(qr)
    it = "u64" if np.dtype(col_fwd.dtype) == np.uint64 else "u32"
    name = {"lstsq": "colpiv_qr_solve_lstsq_in_place", "solve": "colpiv_qr_solve_in_place", "transpose": "colpiv_qr_solve_transpose_in_place"}[mode]
    m, n = qr.shape
    size = min(m, n)
    getattr(lib(), f"libfaer_v0_23_{name}_{it}_{suf}")(_mat(qr[:, :size]), _mat(q_coeff), _mat(qr[:size, :]), C.c_int(0),
                                                     SliceRef(col_fwd.ctypes.data, n), SliceRef(col_bwd.ctypes.data, n), _mat(rhs, MatMut), par,
                                                     MemAlloc(None, 0))
    return rhs


def _it(p):
    return "u64" if np.dtype(p.dtype) == np.uint64 else "u32"


def full_piv_lu_reconstruct(out, lu, row_fwd, row_bwd, col_fwd, col_bwd, par=PAR_SEQ):
    """lu/full_pivoting/reconstruct.rs: out <- P^-1 L U Q^-1"""
    suf, _, _ = _dtype_suffix(lu)
    m, n = lu.shape
    getattr(lib(), f"libfaer_v0_23_full_piv_lu_reconstruct_{_it(row_fwd)}_{suf}")(
        _mat(out, MatMut), _mat(lu), _mat(lu), SliceRef(row_fwd.ctypes.data, m), SliceRef(row_bwd.ctypes.data, m), SliceRef(col_fwd.ctypes.data, n),
        SliceRef(col_bwd.ctypes.data, n), par, MemAlloc(None, 0))
    return out


def full_piv_lu_inverse(out, lu, row_fwd, row_bwd, col_fwd, col_bwd, par=PAR_SEQ):
    """lu/full_pivoting/inverse.rs: out <- A^-1"""
    suf, _, _ = _dtype_suffix(lu)
    n = lu.shape[0]
    getattr(lib(), f"libfaer_v0_23_full_piv_lu_inverse_{_it(row_fwd)}_{suf}")(
        _mat(out, MatMut), _mat(lu), _mat(lu), SliceRef(row_fwd.ctypes.data, n), SliceRef(row_bwd.ctypes.data, n), SliceRef(col_fwd.ctypes.data, n),
        SliceRef(col_bwd.ctypes.data, n), par, MemAlloc(None, 0))
    return out


def colpiv_qr_reconstruct(out, qr, q_coeff, col_fwd, col_bwd, par=PAR_SEQ):
    """qr/col_pivoting/reconstruct.rs: out <- Q R P^-1"""
    suf, _, _ = _dtype_suffix(qr)
    m, n = qr.shape
    size = min(m, n)
    getattr(lib(), f"libfaer_v0_23_colpiv_qr_reconstruct_{_it(col_fwd)}_{suf}")(
        _mat(out, MatMut), _mat(qr[:, :size]), _mat(q_coeff), _mat(qr[:size, :]), SliceRef(col_fwd.ctypes.data, n), SliceRef(col_bwd.ctypes.data, n), par,
        MemAlloc(None, 0))
    return out


def colpiv_qr_inverse(out, qr, q_coeff, col_fwd, col_bwd, par=PAR_SEQ):
    """qr/col_pivoting/inverse.rs: out <- A^-1 (square)"""
    suf, _, _ = _dtype_suffix(qr)
    n = qr.shape[0]
    getattr(lib(), f"libfaer_v0_23_colpiv_qr_inverse_{_it(col_fwd)}_{suf}")(
        _mat(out, MatMut), _mat(qr), _mat(q_coeff), _mat(qr), SliceRef(col_fwd.ctypes.data, n), SliceRef(col_bwd.ctypes.data, n), par, MemAlloc(None, 0))
    return out


BcastFn = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)


IbcastFn = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)
WaitFn = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


class HipComm(C.Structure):
    """include/faer_hip.h FaerHipComm {rank, world_size, bcast, user, ibcast, wait}"""
    _fields_ = [("rank", C.c_int), ("world_size", C.c_int), ("bcast", BcastFn), ("user", C.c_void_p), ("ibcast", IbcastFn),
                ("wait", WaitFn)]


def _make_comm(rank, world_size, panel_ws, bcast, ibcast=None):
    """FaerHipComm over a python transport.  bcast(tensor_view_of_the_device_buffer, root) is blocking (stream ordered);
    ibcast(view, root) may return a handle with .wait() (e.g. torch.distributed.broadcast(..., async_op=True)):
    the library then overlaps the transfer of the next panel with the trailing updates.  Returns (comm, keepalive)."""
    import torch

    ws_bytes = panel_ws.view(torch.uint8)
    base = panel_ws.data_ptr()
    pending = {}

    def cb(user, buf, nbytes, root):
        off = buf - base
        bcast(ws_bytes[off:off + nbytes], root)

    def icb(user, buf, nbytes, root, slot):
        off = buf - base
        pending[slot] = ibcast(ws_bytes[off:off + nbytes], root)

    def wcb(user, slot):
        h = pending.pop(slot, None)
        if h is not None:
            h.wait()

    fns = (BcastFn(cb), IbcastFn(icb) if ibcast else IbcastFn(), WaitFn(wcb) if ibcast else WaitFn())
    return HipComm(int(rank), int(world_size), fns[0], None, fns[1], fns[2]), fns


class RcclTransport:
    """Built-in transport of the distributed drivers (include/faer_hip.h, csrc/rccl_transport.hip): ncclBroadcast on a
    dedicated stream, event-ordered against the caller's stream; no Python callback in the factorization loop.

    Collective: every rank constructs it with the same 128-byte id (rank 0: RcclTransport.unique_id(), shipped to the
    others by the application, e.g. torch.distributed.broadcast of a uint8 tensor)."""

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        rc = lib().faer_hip_rccl_unique_id(buf)
        if rc != 0:
            raise RuntimeError(f"faer_hip_rccl_unique_id failed ({rc}): librccl.so not loadable?")
        return bytes(buf)

    def __init__(self, unique_id, rank, world_size):
        L = lib()
        L.faer_hip_rccl_create.restype = C.c_void_p
        L.faer_hip_rccl_comm.restype = HipComm
        L.faer_hip_rccl_comm.argtypes = [C.c_void_p]
        L.faer_hip_rccl_destroy.argtypes = [C.c_void_p]
        assert len(unique_id) == 128
        self.handle = L.faer_hip_rccl_create((C.c_ubyte * 128).from_buffer_copy(unique_id), int(rank), int(world_size))
        self.comm = L.faer_hip_rccl_comm(C.c_void_p(self.handle))

    def stats(self):
        """{ranks the communicator reports (ncclCommCount), broadcasts, bytes, device ms inside ncclBroadcast} since the last call"""
        out = (C.c_double * 4)()
        L = lib()
        L.faer_hip_rccl_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.faer_hip_rccl_stats(C.c_void_p(self.handle), out)
        return {"ncclCommCount": int(out[0]), "broadcasts": int(out[1]), "bytes": float(out[2]), "bcast_device_ms": float(out[3])}

    def close(self):
        if self.handle:
            lib().faer_hip_rccl_destroy(C.c_void_p(self.handle))
            self.handle = None


class LoopbackGroup:
    """Loop-back transport (csrc/loop_transport.hip, TEST infrastructure): the ranks of a distributed factorization as threads of this
    process on one GPU.  `group.rank(r)` must be called on the thread that runs rank r; the returned object is a `transport=` argument
    of dist_partial_piv_lu / dist_llt (it has the `.comm` of an RcclTransport)."""

    class Rank:
        def __init__(self, group, rank):
            L = lib()
            L.faer_hip_loopback_rank_create.restype = C.c_void_p
            L.faer_hip_loopback_rank_create.argtypes = [C.c_void_p, C.c_int]
            L.faer_hip_loopback_comm.restype = HipComm
            L.faer_hip_loopback_comm.argtypes = [C.c_void_p]
            self.handle = L.faer_hip_loopback_rank_create(C.c_void_p(group.handle), int(rank))
            self.comm = L.faer_hip_loopback_comm(C.c_void_p(self.handle))

        def stats(self):
            out = (C.c_double * 2)()
            L = lib()
            L.faer_hip_loopback_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.faer_hip_loopback_stats(C.c_void_p(self.handle), out)
            return {"broadcasts": int(out[0]), "bytes": float(out[1])}

        def close(self):
            if self.handle:
                L = lib()
                L.faer_hip_loopback_rank_destroy.argtypes = [C.c_void_p]
                L.faer_hip_loopback_rank_destroy(C.c_void_p(self.handle))
                self.handle = None

    def __init__(self, world_size):
        L = lib()
        L.faer_hip_loopback_group_create.restype = C.c_void_p
        self.handle = L.faer_hip_loopback_group_create(C.c_int(int(world_size)))
        self.world_size = int(world_size)

    def rank(self, rank):
        return LoopbackGroup.Rank(self, rank)

    def close(self):
        if self.handle:
            L = lib()
            L.faer_hip_loopback_group_destroy.argtypes = [C.c_void_p]
            L.faer_hip_loopback_group_destroy(C.c_void_p(self.handle))
            self.handle = None


PROF_CLASSES = ("mfma_products", "lu_panel", "qr_update", "qr_gram", "qr_panel", "llt_leaf")
PROF_UNITS = ("flop", "columns", "bytes", "bytes", "launches", "columns")


def prof_begin():
    """Start bracketing the dominant kernel classes of this thread's library calls with timing events (faer_hip.h)."""
    lib().faer_hip_prof_begin()


def prof_end():
    """-> {class: {"ms", "launches", "units", "unit"}} of the launches since prof_begin (synchronises the device)."""
    out = (C.c_double * (3 * len(PROF_CLASSES)))()
    lib().faer_hip_prof_end(out)
    return {name: {"ms": out[3 * i], "launches": int(out[3 * i + 1]), "units": out[3 * i + 2], "unit": PROF_UNITS[i]}
            for i, name in enumerate(PROF_CLASSES)}


def prof_end_spans(cap=8192):
    """prof_end plus one record per profiled launch: (totals, [{"cls", "ms", "units", "d": (d0, d1, d2, d3), "stream", "t0_ms"}])"""
    out = (C.c_double * (3 * len(PROF_CLASSES)))()
    sp = (C.c_double * (8 * cap))()
    L = lib()
    L.faer_hip_prof_end_spans.restype = C.c_size_t
    n = L.faer_hip_prof_end_spans(out, sp, C.c_size_t(cap))
    tot = {name: {"ms": out[3 * i], "launches": int(out[3 * i + 1]), "units": out[3 * i + 2], "unit": PROF_UNITS[i]}
           for i, name in enumerate(PROF_CLASSES)}
    spans = []
    for i in range(n):
        r = sp[8 * i:8 * i + 8]
        d3 = int(r[6])
        spans.append({"cls": PROF_CLASSES[int(r[0])], "ms": r[1], "units": r[2], "d": (int(r[3]), int(r[4]), int(r[5]), d3 & 0xFFFF),
                      "stream": ("caller", "bulk", "panel", "side")[d3 >> 16], "t0_ms": r[7]})
    return tot, spans


def xwg_hop_us(iters=2000):
    """Idle-chip hand-off latency between two workgroups on different XCDs, microseconds per hop (< 0: timed out)."""
    return float(lib().faer_hip_xwg_hop_us(C.c_int(iters)))


def dist_last_stats():
    """the calling thread's last distributed factorization: device ms of the call, of the panels this rank owned, their count"""
    out = (C.c_double * 3)()
    lib().faer_hip_dist_last_stats(out)
    return {"total_device_ms": float(out[0]), "panel_device_ms": float(out[1]), "panels_owned": int(out[2])}


def dist_local_ncols(n, nb, rank, world_size):
    return lib().faer_hip_dist_local_ncols(C.c_size_t(n), C.c_size_t(nb), int(rank), int(world_size))


def dist_partial_piv_lu(a_local, n_global, nb, rank, world_size, bcast=None, panel_ws=None, ibcast=None, transport=None):
    """Distributed partial-pivot LU (1-D block-cyclic columns, one process per GPU; csrc/dist_lu.h).

    a_local  : this rank's block columns (nrows x dist_local_ncols, column major torch cuda tensor), factored in place
    bcast    : callable(torch uint8 tensor viewing the DEVICE broadcast buffer, root) -- the transport, e.g.
               lambda t, root: torch.distributed.broadcast(t, src=root)   (RCCL under the "nccl" backend)
    ibcast   : optional callable(view, root) -> handle with .wait() (async broadcast): enables the overlap of the next
               panel's transfer with the trailing updates
    transport: an RcclTransport instead of the two callables (direct RCCL, no Python in the loop)
    returns  : (perm_fwd, perm_bwd, transposition_count), identical on every rank"""
    import torch

    suf, _, _ = _dtype_suffix(a_local)
    m = a_local.shape[0]
    L = lib()
    dt = DTYPE_F64 if suf == "f64" else DTYPE_F32
    if panel_ws is None:
        nsc = L.faer_hip_dist_panel_ws_scalars(C.c_size_t(m), C.c_size_t(nb), C.c_int(dt))
        panel_ws = torch.empty(nsc, dtype=a_local.dtype, device=a_local.device)
    comm, _keep = (transport.comm, None) if transport is not None else _make_comm(rank, world_size, panel_ws, bcast, ibcast)
    base = panel_ws.data_ptr()
    fwd = np.zeros(m, dtype=np.uint64)
    bwd = np.zeros(m, dtype=np.uint64)
    st = getattr(L, f"faer_hip_dist_partial_piv_lu_{suf}")(_mat(a_local, MatMut), C.c_size_t(n_global), C.c_size_t(nb),
                                                            SliceMut(fwd.ctypes.data, m), SliceMut(bwd.ctypes.data, m), comm,
                                                            C.c_void_p(base))
    if st.tag != 0:
        raise RuntimeError("PartialPivLuStatus::Unknown")
    return fwd, bwd, st.transposition_count


def dist_llt(a_local, n_global, nb, rank, world_size, bcast=None, panel_ws=None, ibcast=None, regularization=(0.0, 0.0), transport=None):
    """Distributed Cholesky (lower; 1-D block-cyclic columns, one process per GPU; csrc/dist_llt.h).

    a_local : this rank's block columns at full height (n x dist_local_ncols, column major torch cuda tensor)
    returns : dynamic_regularization_count; raises LltError(index) (same index on every rank)"""
    import torch

    suf, ct, _ = _dtype_suffix(a_local)
    L = lib()
    dt = DTYPE_F64 if suf == "f64" else DTYPE_F32
    if panel_ws is None:
        L.faer_hip_dist_llt_ws_scalars.restype = C.c_size_t
        nsc = L.faer_hip_dist_llt_ws_scalars(C.c_size_t(n_global), C.c_size_t(nb), C.c_int(dt))
        panel_ws = torch.empty(nsc, dtype=a_local.dtype, device=a_local.device)
    comm, _keep = (transport.comm, None) if transport is not None else _make_comm(rank, world_size, panel_ws, bcast, ibcast)
    delta, eps = ct(regularization[0]), ct(regularization[1])
    reg = LltRegularization(C.cast(C.pointer(delta), C.c_void_p), C.cast(C.pointer(eps), C.c_void_p))
    fn = getattr(L, f"faer_hip_dist_llt_{suf}")
    fn.restype = LltStatus
    st = fn(_mat(a_local, MatMut), C.c_size_t(n_global), C.c_size_t(nb), reg, comm, C.c_void_p(panel_ws.data_ptr()))
    if st.tag == 0:
        return st.value
    if st.tag == 1:
        raise LltError(st.value)
    raise RuntimeError("LltStatus::Unknown")


def qr_recommended_block_size(nrows, ncols, dtype=np.float64):
    suf = "f64" if np.dtype(dtype) == np.float64 else "f32"
    return getattr(lib(), f"libfaer_v0_23_qr_recommended_block_size_{suf}")(C.c_size_t(nrows), C.c_size_t(ncols))


def qr_factor_in_place(a, q_coeff, par=PAR_SEQ):
    """q_coeff: block_size x min(m, n).  returns rank (QrInfo.rank)"""
    suf, _, _ = _dtype_suffix(a)
    L = lib()
    params = getattr(L, f"libfaer_v0_23_QrParams_{suf}")()
    st = getattr(L, f"libfaer_v0_23_qr_factor_in_place_{suf}")(_mat(a, MatMut), _mat(q_coeff, MatMut), par,
                                                             MemAlloc(None, 0), params)
    if st.tag != 0:
        raise RuntimeError("QrStatus::Unknown")
    return st.rank


def apply_block_householder_sequence_on_the_left_in_place(basis, factor, rhs, transpose=False, par=PAR_SEQ):
    suf, _, _ = _dtype_suffix(rhs)
    name = "apply_householder_transpose_on_the_left" if transpose else "apply_householder_on_the_left"
    getattr(lib(), f"libfaer_v0_23_{name}_{suf}")(_mat(basis), _mat(factor), C.c_int(CONJ_NO), _mat(rhs, MatMut), par,
                                                MemAlloc(None, 0))
    return rhs


def apply_block_householder_sequence_on_the_right_in_place(basis, factor, matrix, transpose=False, par=PAR_SEQ):
    """householder.rs:813-854: matrix <- matrix Q (or matrix Q^H)"""
    suf, _, _ = _dtype_suffix(matrix)
    name = "apply_householder_transpose_on_the_right" if transpose else "apply_householder_on_the_right"
    getattr(lib(), f"libfaer_v0_23_{name}_{suf}")(_mat(basis), _mat(factor), C.c_int(CONJ_NO), _mat(matrix, MatMut), par,
                                                MemAlloc(None, 0))
    return matrix


def _diag_vec(ld):
    n = ld.shape[0]
    if _is_torch(ld):
        return VecRef(ld.data_ptr(), n, ld.stride(0) + ld.stride(1))
    return VecRef(ld.ctypes.data, n, (ld.strides[0] + ld.strides[1]) // ld.itemsize)


def inverse_triangular_in_place(t_inv, t, upper=False, unit=False, par=PAR_SEQ):
    """triangular_inverse.rs: the (unit) lower / upper triangle of t_inv <- inverse of the triangle of t; the rest of
    t_inv (and, unit: its diagonal) is left untouched.  float32 / float64 and complex64 / complex128 (interleaved); the other
    triangle of t (and, unit: its diagonal) is never read"""
    suf, _, _ = _dtype_suffix(t)
    name = f"inverse_{'unit_' if unit else ''}triangular_{'upper' if upper else 'lower'}_in_place"
    getattr(lib(), f"libfaer_v0_23_{name}_{suf}")(_mat(t_inv, MatMut), _mat(t), par)
    return t_inv


def llt_reconstruct(out, l, par=PAR_SEQ):
    """cholesky/llt/reconstruct.rs: lower(out) <- L L^H"""
    suf, _, _ = _dtype_suffix(l)
    getattr(lib(), f"libfaer_v0_23_llt_reconstruct_{suf}")(_mat(out, MatMut), _mat(l), par, MemAlloc(None, 0))
    return out


def llt_inverse(out, l, par=PAR_SEQ):
    """cholesky/llt/inverse.rs: lower(out) <- (L L^H)^-1"""
    suf, _, _ = _dtype_suffix(l)
    getattr(lib(), f"libfaer_v0_23_llt_inverse_{suf}")(_mat(out, MatMut), _mat(l), par, MemAlloc(None, 0))
    return out


def ldlt_reconstruct(out, ld, par=PAR_SEQ):
    """cholesky/ldlt/reconstruct.rs with L and D packed as ldlt_factor_in_place leaves them: lower(out) <- L D L^H"""
    suf, _, _ = _dtype_suffix(ld)
    getattr(lib(), f"libfaer_v0_23_ldlt_reconstruct_{suf}")(_mat(out, MatMut), _mat(ld), _diag_vec(ld), par, MemAlloc(None, 0))
    return out


def ldlt_inverse(out, ld, par=PAR_SEQ):
    """cholesky/ldlt/inverse.rs: lower(out) <- (L D L^H)^-1"""
    suf, _, _ = _dtype_suffix(ld)
    getattr(lib(), f"libfaer_v0_23_ldlt_inverse_{suf}")(_mat(out, MatMut), _mat(ld), _diag_vec(ld), par, MemAlloc(None, 0))
    return out


def partial_piv_lu_reconstruct(out, lu, perm_fwd, perm_bwd, par=PAR_SEQ):
    """lu/partial_pivoting/reconstruct.rs: out <- P^-1 L U (`lu` holds L and U packed, any m x n)"""
    suf, _, _ = _dtype_suffix(lu)
    it = "u64" if np.dtype(perm_fwd.dtype) == np.uint64 else "u32"
    m = lu.shape[0]
    getattr(lib(), f"libfaer_v0_23_partial_piv_lu_reconstruct_{it}_{suf}")(
        _mat(out, MatMut), _mat(lu), _mat(lu), SliceRef(perm_fwd.ctypes.data, m), SliceRef(perm_bwd.ctypes.data, m), par, MemAlloc(None, 0))
    return out


def partial_piv_lu_inverse(out, lu, perm_fwd, perm_bwd, par=PAR_SEQ):
    """lu/partial_pivoting/inverse.rs: out <- A^-1"""
    suf, _, _ = _dtype_suffix(lu)
    it = "u64" if np.dtype(perm_fwd.dtype) == np.uint64 else "u32"
    n = lu.shape[0]
    getattr(lib(), f"libfaer_v0_23_partial_piv_lu_inverse_{it}_{suf}")(
        _mat(out, MatMut), _mat(lu), _mat(lu), SliceRef(perm_fwd.ctypes.data, n), SliceRef(perm_bwd.ctypes.data, n), par, MemAlloc(None, 0))
    return out


def qr_reconstruct(out, qr, q_coeff, par=PAR_SEQ):
    """qr/no_pivoting/reconstruct.rs: out <- Q R (`qr` holds the Householder basis below the diagonal and R on / above it)"""
    suf, _, _ = _dtype_suffix(qr)
    m, n = qr.shape
    size = min(m, n)
    getattr(lib(), f"libfaer_v0_23_qr_reconstruct_{suf}")(_mat(out, MatMut), _mat(qr[:, :size]), _mat(q_coeff), _mat(qr[:size, :]), par,
                                                        MemAlloc(None, 0))
    return out


def qr_inverse(out, qr, q_coeff, par=PAR_SEQ):
    """qr/no_pivoting/inverse.rs: out <- A^-1 (square)"""
    suf, _, _ = _dtype_suffix(qr)
    getattr(lib(), f"libfaer_v0_23_qr_inverse_{suf}")(_mat(out, MatMut), _mat(qr), _mat(q_coeff), _mat(qr), par, MemAlloc(None, 0))
    return out


def _vec(x, cls=VecRef):
    """1-D numpy array / torch tensor -> VecRef/VecMut (stride in elements)"""
    if _is_torch(x):
        assert x.dim() == 1
        return cls(x.data_ptr(), x.shape[0], x.stride(0))
    assert x.ndim == 1
    return cls(x.ctypes.data, x.shape[0], x.strides[0] // x.itemsize)


def lblt_factor_in_place(a, subdiag=None, pivoting=None, index_dtype=np.uint64, par=PAR_SEQ):
    """cholesky/bunch_kaufman/factor.rs:1161-1234: P A P^T = L B L^T of the symmetric matrix in the lower triangle of `a` (the strict
    upper triangle is never touched).  Unit lower L strictly below the diagonal of `a`, the diagonal of B on it, the subdiagonal of
    the 2 x 2 blocks in `subdiag` (created next to `a` when None).  pivoting: a PIVOTING_* constant or a key of PivotingStrategy
    ("partial", ..., "full"; None: the default, PartialDiag).  A value the library does not run raises ValueError (the C entry point
    would abort).  returns (subdiag, perm_fwd, perm_bwd, transposition_count)"""
    suf, _, _ = _dtype_suffix(a)
    n = a.shape[0]
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    if subdiag is None:
        if _is_torch(a):
            import torch

            subdiag = torch.zeros(n, dtype=a.dtype, device=a.device)
        else:
            subdiag = np.zeros(n, dtype=a.dtype)
    fwd = np.zeros(n, dtype=index_dtype)
    bwd = np.zeros(n, dtype=index_dtype)
    L = lib()
    params = getattr(L, f"libfaer_v0_23_LbltParams_{suf}")()
    if pivoting is not None:
        params.pivoting = PivotingStrategy[pivoting] if isinstance(pivoting, str) else int(pivoting)
        if not lblt_pivoting_supported(params.pivoting):
            raise ValueError(f"lblt_factor_in_place: unsupported pivoting strategy {pivoting!r}")
    st = getattr(L, f"libfaer_v0_23_lblt_factor_in_place_{it}_{suf}")(
        _mat(a, MatMut), _vec(subdiag, VecMut), SliceMut(fwd.ctypes.data, n), SliceMut(bwd.ctypes.data, n), par, MemAlloc(None, 0), params)
    if st.tag != 0:
        raise RuntimeError("LbltStatus::Unknown")
    return subdiag, fwd, bwd, st.transposition_count


def lblt_pivoting_supported(pivoting):
    """1 if lblt_factor_in_place runs the FaerPivotingStrategy value `pivoting` (an int or a key of PivotingStrategy), else 0; no GPU call"""
    if isinstance(pivoting, str):
        pivoting = PivotingStrategy.get(pivoting, -1)
    return int(lib().faer_hip_lblt_pivoting_supported(C.c_int(int(pivoting))))


def _lblt_call(name, lb, diag, subdiag, perm_fwd, perm_bwd):
    suf, _, _ = _dtype_suffix(lb)
    it = "u64" if np.dtype(perm_fwd.dtype) == np.uint64 else "u32"
    n = lb.shape[0]
    d = _diag_vec(lb) if diag is None else _vec(diag)
    return getattr(lib(), f"libfaer_v0_23_{name}_{it}_{suf}"), d, _vec(subdiag), SliceRef(perm_fwd.ctypes.data, n), SliceRef(perm_bwd.ctypes.data, n)


def lblt_solve_in_place(lb, subdiag, perm_fwd, perm_bwd, rhs, diag=None, par=PAR_SEQ):
    """cholesky/bunch_kaufman/solve.rs:35-104: rhs <- A^-1 rhs; `lb` as lblt_factor_in_place leaves it (diag None: its diagonal)"""
    fn, d, s, pf, pb = _lblt_call("lblt_solve_in_place", lb, diag, subdiag, perm_fwd, perm_bwd)
    fn(_mat(lb), d, s, C.c_int(CONJ_NO), pf, pb, _mat(rhs, MatMut), par, MemAlloc(None, 0))
    return rhs


def lblt_reconstruct(out, lb, subdiag, perm_fwd, perm_bwd, diag=None, par=PAR_SEQ):
    """cholesky/bunch_kaufman/reconstruct.rs: lower(out) <- P^T L B L^T P"""
    fn, d, s, pf, pb = _lblt_call("lblt_reconstruct", lb, diag, subdiag, perm_fwd, perm_bwd)
    fn(_mat(out, MatMut), _mat(lb), d, s, pf, pb, par, MemAlloc(None, 0))
    return out


def lblt_inverse(out, lb, subdiag, perm_fwd, perm_bwd, diag=None, par=PAR_SEQ):
    """cholesky/bunch_kaufman/inverse.rs: out <- A^-1 (the whole matrix)"""
    fn, d, s, pf, pb = _lblt_call("lblt_inverse", lb, diag, subdiag, perm_fwd, perm_bwd)
    fn(_mat(out, MatMut), _mat(lb), d, s, pf, pb, par, MemAlloc(None, 0))
    return out


def debug_lblt_last():
    """(blocked panels, leaf rows, 2 x 2 pivots, host synchronisations inside panels) of this thread's last lblt_factor_in_place;
    for the Full strategy (pivot steps of the multi-workgroup path, rows finished by the leaf, 2 x 2 pivots, host synchronisations
    before the leaf)"""
    out = (C.c_size_t * 4)()
    lib().faer_hip_debug_lblt_last(out)
    return tuple(int(v) for v in out)


def piv_llt_factor_in_place(a, index_dtype=np.uint64, par=PAR_SEQ, raise_on_error=True):
    """cholesky/llt_pivoting/factor.rs:47-199: P A P^T = L L^T of the symmetric positive semidefinite matrix in the lower triangle of
    `a` (the strict upper triangle is never touched); L replaces the lower triangle.  returns (perm_fwd, perm_bwd, rank,
    transposition_count).  NonPositivePivot raises LltError, or with raise_on_error=False the PivLltStatus is returned instead."""
    suf, _, _ = _dtype_suffix(a)
    n = a.shape[0]
    it = "u64" if np.dtype(index_dtype) == np.uint64 else "u32"
    fwd = np.zeros(n, dtype=index_dtype)
    bwd = np.zeros(n, dtype=index_dtype)
    L = lib()
    params = getattr(L, f"libfaer_v0_23_PivLltParams_{suf}")()
    st = getattr(L, f"libfaer_v0_23_piv_llt_factor_in_place_{it}_{suf}")(
        _mat(a, MatMut), SliceMut(fwd.ctypes.data, n), SliceMut(bwd.ctypes.data, n), par, MemAlloc(None, 0), params)
    if st.tag != PIV_LLT_OK:
        if not raise_on_error:
            return st
        if st.tag == PIV_LLT_NON_POSITIVE_PIVOT:
            raise LltError(st.index)
        raise RuntimeError("PivLltStatus::Unknown")
    return fwd, bwd, st.rank, st.transposition_count


def _piv_llt_call(name, l, perm_fwd, perm_bwd):
    suf, _, _ = _dtype_suffix(l)
    it = "u64" if np.dtype(perm_fwd.dtype) == np.uint64 else "u32"
    n = l.shape[0]
    return getattr(lib(), f"libfaer_v0_23_{name}_{it}_{suf}"), SliceRef(perm_fwd.ctypes.data, n), SliceRef(perm_bwd.ctypes.data, n)


def piv_llt_solve_in_place(l, perm_fwd, perm_bwd, rhs, par=PAR_SEQ):
    """cholesky/llt_pivoting/solve.rs:13-41: rhs <- A^-1 rhs; `l` as a full-rank piv_llt_factor_in_place leaves it"""
    fn, pf, pb = _piv_llt_call("piv_llt_solve_in_place", l, perm_fwd, perm_bwd)
    fn(_mat(l), pf, pb, C.c_int(CONJ_NO), _mat(rhs, MatMut), par, MemAlloc(None, 0))
    return rhs


def piv_llt_reconstruct(out, l, perm_fwd, perm_bwd, par=PAR_SEQ):
    """cholesky/llt_pivoting/reconstruct.rs: lower(out) <- P^T L L^T P"""
    fn, pf, pb = _piv_llt_call("piv_llt_reconstruct", l, perm_fwd, perm_bwd)
    fn(_mat(out, MatMut), _mat(l), pf, pb, par, MemAlloc(None, 0))
    return out


def piv_llt_inverse(out, l, perm_fwd, perm_bwd, par=PAR_SEQ):
    """cholesky/llt_pivoting/inverse.rs: lower(out) <- A^-1"""
    fn, pf, pb = _piv_llt_call("piv_llt_inverse", l, perm_fwd, perm_bwd)
    fn(_mat(out, MatMut), _mat(l), pf, pb, par, MemAlloc(None, 0))
    return out


def debug_piv_llt_last():
    """(blocked panels, leaf rows, columns factored, host synchronisations inside panels) of this thread's last piv_llt_factor_in_place"""
    out = (C.c_size_t * 4)()
    lib().faer_hip_debug_piv_llt_last(out)
    return tuple(int(v) for v in out)


def debug_clu_shape(dtype):
    """(W, leaf_rows) of the complex partial-pivot LU: columns per panel and the row count of the tallest panel its LDS-resident leaf
    takes; dtype complex64 or complex128.  Needs no GPU."""
    out = (C.c_size_t * 2)()
    lib().faer_hip_debug_clu_shape(C.c_int(DTYPE_C64 if np.dtype(dtype) == np.complex128 else DTYPE_C32), out)
    return int(out[0]), int(out[1])


def debug_clu_last():
    """{panels on the LDS leaf, panels on the column-step kernels, column-step launches, interchange launches} of this thread's last
    complex partial_piv_lu_factor_in_place"""
    out = (C.c_size_t * 4)()
    lib().faer_hip_debug_clu_last(out)
    return dict(zip(("leaf_panels", "step_panels", "step_launches", "swap_launches"), (int(v) for v in out)))


def debug_ctrtri_shape(dtype):
    """(E, sub_blocks) of the complex triangular inverse: the edge of its LDS-resident leaf and the number of sub-blocks along that
    edge (the leaf inverts E // sub_blocks-wide diagonal sub-blocks by substitution and combines them by doubling); dtype complex64 or
    complex128.  Needs no GPU."""
    out = (C.c_size_t * 2)()
    lib().faer_hip_debug_ctrtri_shape(C.c_int(np.dtype(dtype).itemsize), out)
    return int(out[0]), int(out[1])


def debug_scratch_fill(byte=-1):
    """tests: from now on every device scratch buffer the library hands to itself is first filled, over its whole pool size, with
    `byte` (0 .. 255); -1 switches the fill off again (the default).  Process wide; resets debug_scratch_fill_stats."""
    lib().faer_hip_debug_scratch_fill(C.c_int(int(byte)))


def debug_scratch_fill_stats():
    """(fills, bytes filled) since the last debug_scratch_fill"""
    out = (C.c_size_t * 2)()
    lib().faer_hip_debug_scratch_fill_stats(out)
    return int(out[0]), int(out[1])


# ------------------------------------------------------------------ high level owners (faer/src/linalg/solvers.rs)
def _empty_like_f(a, shape):
    if _is_torch(a):
        import torch

        return torch.zeros(shape[::-1], dtype=a.dtype, device=a.device).t()  # column major
    return np.zeros(shape, dtype=a.dtype, order="F")


def _copy_f(a):
    if _is_torch(a):
        return a.t().contiguous().t()
    return np.array(a, order="F", copy=True)


def partial_piv_lu_solve_in_place(lu, perm_fwd, perm_bwd, rhs, transpose=False, par=PAR_SEQ, conj=False):
    """lu/partial_pivoting/solve.rs:20-80: rhs <- op(A)^-1 rhs (or op(A)^-T rhs); `lu` holds L (unit lower) and U packed.
    conj: op is the conjugate (complex scalars; the real entry points ignore it)"""
    suf, _, _ = _dtype_suffix(lu)
    it = "u64" if np.dtype(perm_fwd.dtype) == np.uint64 else "u32"
    name = "partial_piv_lu_solve_transpose_in_place" if transpose else "partial_piv_lu_solve_in_place"
    n = lu.shape[0]
    getattr(lib(), f"libfaer_v0_23_{name}_{it}_{suf}")(
        _mat(lu), _mat(lu), C.c_int(CONJ_YES if conj else CONJ_NO), SliceRef(perm_fwd.ctypes.data, n), SliceRef(perm_bwd.ctypes.data, n), _mat(rhs, MatMut), par,
        MemAlloc(None, 0))
    return rhs


def qr_solve_lstsq_in_place(qr, q_coeff, rhs, par=PAR_SEQ):
    """qr/no_pivoting/solve.rs:38-75: the least squares solution ends in the top ncols rows of rhs"""
    suf, _, _ = _dtype_suffix(qr)
    getattr(lib(), f"libfaer_v0_23_qr_solve_lstsq_in_place_{suf}")(_mat(qr), _mat(q_coeff), _mat(qr), C.c_int(0), _mat(rhs, MatMut), par,
                                                                   MemAlloc(None, 0))
    return rhs


def qr_solve_in_place(qr, q_coeff, rhs, transpose=False, par=PAR_SEQ):
    """qr/no_pivoting/solve.rs:98-175: square systems, rhs <- A^-1 rhs or A^-T rhs"""
    suf, _, _ = _dtype_suffix(qr)
    name = "qr_solve_transpose_in_place" if transpose else "qr_solve_in_place"
    getattr(lib(), f"libfaer_v0_23_{name}_{suf}")(_mat(qr), _mat(q_coeff), _mat(qr), C.c_int(0), _mat(rhs, MatMut), par, MemAlloc(None, 0))
    return rhs


class Llt:
    """solvers.rs:770-817: copies the lower triangle, factors, zeroes the strict upper triangle."""

    def __init__(self, a):
        self.l = _copy_f(a)
        llt_factor_in_place(self.l)
        if _is_torch(self.l):
            self.l.copy_(self.l.tril())
        else:
            self.l[:] = np.tril(self.l)

    def L(self):
        return self.l

    def solve_in_place(self, rhs):
        return llt_solve_in_place(self.l, rhs)


class Lblt:
    """solvers.rs Lblt: copies the matrix, factors its lower triangle with the default strategy, or with `pivoting` (as
    lblt_factor_in_place takes it)"""

    def __init__(self, a, pivoting=None):
        self.lb = _copy_f(a)
        self.subdiag, self.perm, self.perm_inv, self.transposition_count = lblt_factor_in_place(self.lb, pivoting=pivoting)

    def solve_in_place(self, rhs):
        return lblt_solve_in_place(self.lb, self.subdiag, self.perm, self.perm_inv, rhs)

    def reconstruct(self):
        out = _empty_like_f(self.lb, self.lb.shape)
        return lblt_reconstruct(out, self.lb, self.subdiag, self.perm, self.perm_inv)

    def inverse(self):
        out = _empty_like_f(self.lb, self.lb.shape)
        return lblt_inverse(out, self.lb, self.subdiag, self.perm, self.perm_inv)


class PartialPivLu:
    """solvers.rs:955-1035"""

    def __init__(self, a):
        self.lu = _copy_f(a)
        self.perm, self.perm_inv, self.transposition_count = partial_piv_lu_factor_in_place(self.lu)

    def solve_in_place(self, rhs):
        return partial_piv_lu_solve_in_place(self.lu, self.perm, self.perm_inv, rhs)

    def solve_transpose_in_place(self, rhs):
        return partial_piv_lu_solve_in_place(self.lu, self.perm, self.perm_inv, rhs, transpose=True)


class Qr:
    """solvers.rs:1106-1204"""

    def __init__(self, a):
        m, n = a.shape
        self.qr = _copy_f(a)
        bs = qr_recommended_block_size(m, n, np.float64 if _dtype_suffix(a)[0] == "f64" else np.float32)
        self.q_coeff = _empty_like_f(a, (bs, min(m, n)))
        self.rank = qr_factor_in_place(self.qr, self.q_coeff)

    def Q_basis(self):
        return self.qr

    def Q_coeff(self):
        return self.q_coeff

    def solve_lstsq_in_place(self, rhs):
        return qr_solve_lstsq_in_place(self.qr, self.q_coeff, rhs)
