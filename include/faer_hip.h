/*
 * faer_hip.h -- C ABI of libfaer_hip.so, the MI355X (gfx950) dense backend for faer.
 *
 * Two boundaries are exported:
 *
 *  1. INNER boundary: faer_hip_gemm() has the argument list of
 *     private_gemm_x86::gemm, the third-party kernel faer calls at
 *       faer/src/linalg/matmul/mod.rs:1373-1411            (DstKind::Full)
 *       faer/src/linalg/matmul/triangular.rs:641-680       (DstKind::Lower)
 *       faer/src/linalg/matmul/internal/mod.rs:143-201     (row/col idx + diag)
 *     minus the x86 `InstrSet` argument.  A 3-site #[cfg(feature = "hip")]
 *     patch in faer routes every O(n^3) flop of every decomposition here
 *     (INTEGRATION.md).
 *
 *  2. OUTER boundary: the f32/f64 subset of faer-ffi's C ABI
 *     (faer-ffi/src/lib.rs, generated header faer-ffi/faer.h) with identical
 *     repr(C) struct layouts and identical symbol names
 *     (libfaer_v0_23_<fn>_<dtype>, index-typed ones libfaer_v0_23_<fn>_<u32|u64>_<dtype>),
 *     so a C/C++ client of faer-ffi links against libfaer_hip.so unchanged and
 *     gets whole factorizations executed on the GPU.
 *
 * Pointers: every matrix / slice pointer may be HOST memory (a faer::Mat) or
 * DEVICE memory (hipMalloc / a torch tensor).  The library asks the HIP runtime
 * (hipPointerGetAttributes) and stages host operands through device buffers;
 * device operands are used in place with no copy.  Strides are in ELEMENTS and
 * may be negative or non-unit (faer/src/mat/mod.rs:7-13).
 *
 * Errors: like faer (which panics across extern "C" on precondition
 * violations, faer-ffi/src/lib.rs) a violated precondition or a HIP runtime
 * failure prints a message to stderr and abort()s; numerical failure is
 * reported by value through the *Status unions.  There is NO CPU fallback: if
 * no gfx950 device is usable every compute entry point aborts.
 */
#ifndef FAER_HIP_H
#define FAER_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FAER_HIP_API __attribute__((visibility("default")))

/* ---- repr(C) structs: field-for-field faer-ffi/src/lib.rs:12-113 (faer.h:203-258) ---- */
typedef struct FaerMatRef { const void *ptr; size_t nrows; size_t ncols; ptrdiff_t row_stride; ptrdiff_t col_stride; } FaerMatRef;
typedef struct FaerMatMut { void *ptr; size_t nrows; size_t ncols; ptrdiff_t row_stride; ptrdiff_t col_stride; } FaerMatMut;
typedef struct FaerVecRef { const void *ptr; size_t len; ptrdiff_t stride; } FaerVecRef;
typedef struct FaerVecMut { void *ptr; size_t len; ptrdiff_t stride; } FaerVecMut;
/* len is an ELEMENT count (faer-ffi/src/lib.rs:251-258) */
typedef struct FaerSliceRef { const void *ptr; size_t len; } FaerSliceRef;
typedef struct FaerSliceMut { void *ptr; size_t len; } FaerSliceMut;

typedef enum FaerAccum { FaerAccum_Replace = 0, FaerAccum_Add = 1 } FaerAccum;          /* lib.rs:59-64 */
typedef enum FaerConj { FaerConj_No = 0, FaerConj_Yes = 1 } FaerConj;                   /* lib.rs:65-70 */
typedef enum FaerParTag { FaerParTag_Seq = 0, FaerParTag_Rayon = 1 } FaerParTag;        /* lib.rs:71-76 */
typedef struct FaerPar { FaerParTag tag; size_t nthreads; } FaerPar;                    /* lib.rs:77-82 */
typedef enum FaerBlock {                                                                 /* lib.rs:83-93 */
	FaerBlock_Rectangular = 0,
	FaerBlock_TriangularLower = 1,
	FaerBlock_TriangularUpper = 2,
	FaerBlock_StrictTriangularLower = 3,
	FaerBlock_StrictTriangularUpper = 4,
	FaerBlock_UnitTriangularLower = 5,
	FaerBlock_UnitTriangularUpper = 6
} FaerBlock;
typedef struct FaerLayout { size_t len_bytes; size_t align_bytes; } FaerLayout;          /* lib.rs:94-99 */
typedef struct FaerMemAlloc { void *ptr; size_t len_bytes; } FaerMemAlloc;               /* lib.rs:108-113 */

/* status unions: faer-ffi/src/lib.rs:552-595 + cerr! (:372-407), faer.h:383-469 */
typedef enum FaerLltStatus_Tag { FaerLltStatus_Ok = 0, FaerLltStatus_NonPositivePivot = 1, FaerLltStatus_Unknown = 2 } FaerLltStatus_Tag;
typedef struct FaerLltStatus {
	FaerLltStatus_Tag tag;
	union {
		struct { size_t dynamic_regularization_count; } ok;
		struct { size_t index; } non_positive_pivot;
	};
} FaerLltStatus;
typedef enum FaerPartialPivLuStatus_Tag { FaerPartialPivLuStatus_Ok = 0, FaerPartialPivLuStatus_Unknown = 1 } FaerPartialPivLuStatus_Tag;
typedef struct FaerPartialPivLuStatus {
	FaerPartialPivLuStatus_Tag tag;
	union { struct { size_t transposition_count; } ok; };
} FaerPartialPivLuStatus;
typedef enum FaerQrStatus_Tag { FaerQrStatus_Ok = 0, FaerQrStatus_Unknown = 1 } FaerQrStatus_Tag;
typedef struct FaerQrStatus {
	FaerQrStatus_Tag tag;
	union { struct { size_t rank; } ok; };
} FaerQrStatus;

/* params: faer-ffi/src/lib.rs:650-690 (cparams!) */
typedef struct FaerLltParams { size_t recursion_threshold; size_t block_size; } FaerLltParams;
typedef struct FaerLdltParams { size_t recursion_threshold; size_t block_size; } FaerLdltParams; /* lib.rs:660-664 */
/* lib.rs:572-575, faer.h:346-366: Ok{dynamic_regularization_count} | ZeroPivot{index} | Unknown */
typedef enum FaerLdltStatus_Tag { FaerLdltStatus_Ok = 0, FaerLdltStatus_ZeroPivot = 1, FaerLdltStatus_Unknown = 2 } FaerLdltStatus_Tag;
typedef struct FaerLdltStatus {
	FaerLdltStatus_Tag tag;
	union {
		struct { size_t dynamic_regularization_count; } ok;
		struct { size_t index; } zero_pivot;
	};
} FaerLdltStatus;
typedef struct FaerPartialPivLuParams { size_t recursion_threshold; size_t block_size; size_t par_threshold; } FaerPartialPivLuParams;
typedef struct FaerFullPivLuParams { size_t par_threshold; } FaerFullPivLuParams;
typedef struct FaerColPivQrParams { size_t blocking_threshold; size_t par_threshold; } FaerColPivQrParams;
typedef enum FaerColPivQrStatus_Tag { FaerColPivQrStatus_Ok = 0, FaerColPivQrStatus_Unknown = 1 } FaerColPivQrStatus_Tag;
typedef struct FaerColPivQrStatus {
	FaerColPivQrStatus_Tag tag;
	union {
		struct { size_t transposition_count; } ok;
	};
} FaerColPivQrStatus;
typedef enum FaerFullPivLuStatus_Tag { FaerFullPivLuStatus_Ok = 0, FaerFullPivLuStatus_Unknown = 1 } FaerFullPivLuStatus_Tag;
typedef struct FaerFullPivLuStatus {
	FaerFullPivLuStatus_Tag tag;
	union {
		struct { size_t transposition_count; } ok;
	};
} FaerFullPivLuStatus;
typedef struct FaerQrParams { size_t blocking_threshold; size_t par_threshold; } FaerQrParams;
/* self-adjoint EVD: faer.h:191-194, :260-279, lib.rs:2368-2400 (evd/mod.rs:82-88, evd/tridiag.rs:15-20) */
typedef enum FaerComputeEigenvectors { FaerComputeEigenvectors_No = 0, FaerComputeEigenvectors_Yes = 1 } FaerComputeEigenvectors;
typedef struct FaerTridiagParams { size_t par_threshold; } FaerTridiagParams;
typedef struct FaerSelfAdjointEvdParams { FaerTridiagParams tridiag; size_t recursion_threshold; } FaerSelfAdjointEvdParams;
typedef enum FaerEvdStatus_Tag { FaerEvdStatus_Ok = 0, FaerEvdStatus_NoConvergence = 1 } FaerEvdStatus_Tag;
typedef struct FaerEvdStatus {
	FaerEvdStatus_Tag tag;
	union {
		struct { size_t padding; } ok;
		struct { size_t padding; } no_convergence;
	};
} FaerEvdStatus;
/* general EVD: faer.h:106-126, lib.rs:2402-2457 (evd/hessenberg.rs:8-25, evd/schur/mod.rs:5-36, evd/mod.rs:38-81) */
typedef struct FaerEvdFromSchurParams { size_t recursion_threshold; } FaerEvdFromSchurParams;
typedef struct FaerHessenbergParams { size_t par_threshold; size_t blocking_threshold; } FaerHessenbergParams;
typedef struct FaerSchurParams {
	size_t (*recommended_shift_count)(size_t matrix_dimension, size_t active_block_dimension);
	size_t (*recommended_deflation_window)(size_t matrix_dimension, size_t active_block_dimension);
	size_t blocking_threshold;
	size_t nibble_threshold;
} FaerSchurParams;
typedef struct FaerEvdParams { FaerHessenbergParams hessenberg; FaerSchurParams schur; FaerEvdFromSchurParams evd_from_schur; } FaerEvdParams;
/* generalized EVD: faer.h:132-154, :303-322, lib.rs:2459-2520 (gevd/gen_hessenberg/mod.rs, gevd/mod.rs:37-122) */
typedef struct FaerGeneralizedHessenbergParams { size_t block_size; size_t blocking_threshold; } FaerGeneralizedHessenbergParams;
typedef struct FaerGeneralizedSchurParams {
	size_t (*relative_cost_estimate_of_shift_chase_to_matmul)(size_t matrix_dimension, size_t active_block_dimension);
	size_t (*recommended_shift_count)(size_t matrix_dimension, size_t active_block_dimension);
	size_t (*recommended_deflation_window)(size_t matrix_dimension, size_t active_block_dimension);
	size_t blocking_threshold;
	size_t nibble_threshold;
} FaerGeneralizedSchurParams;
typedef struct FaerGevdFromSchurParams { size_t padding; } FaerGevdFromSchurParams;
typedef struct FaerGevdParams { FaerGeneralizedHessenbergParams hessenberg; FaerGeneralizedSchurParams schur; FaerGevdFromSchurParams evd_from_schur; } FaerGevdParams;
typedef enum FaerGevdStatus_Tag { FaerGevdStatus_Ok = 0, FaerGevdStatus_NoConvergence = 1 } FaerGevdStatus_Tag;
typedef struct FaerGevdStatus {
	FaerGevdStatus_Tag tag;
	union {
		struct { size_t padding; } ok;
		struct { size_t padding; } no_convergence;
	};
} FaerGevdStatus;
/* SVD: faer.h:87-99, :196-201, :471-490, lib.rs:2327-2366 (svd/mod.rs:22-56, svd/bidiag.rs) */
typedef enum FaerComputeSvdVectors { FaerComputeSvdVectors_No = 0, FaerComputeSvdVectors_Thin = 1, FaerComputeSvdVectors_Full = 2 } FaerComputeSvdVectors;
typedef struct FaerBidiagParams { size_t par_threshold; } FaerBidiagParams;
typedef struct FaerSvdParams { FaerBidiagParams bidiag; FaerQrParams qr; size_t recursion_threshold; double qr_ratio_threshold; } FaerSvdParams;
typedef enum FaerSvdStatus_Tag { FaerSvdStatus_Ok = 0, FaerSvdStatus_NoConvergence = 1 } FaerSvdStatus_Tag;
typedef struct FaerSvdStatus {
	FaerSvdStatus_Tag tag;
	union {
		struct { size_t padding; } ok;
		struct { size_t padding; } no_convergence;
	};
} FaerSvdStatus;
/* LBLT (Bunch-Kaufman): faer.h:32-55, :156-160, :324-338, lib.rs:509-548, :576, :665 (cholesky/bunch_kaufman/factor.rs:8-36) */
typedef enum FaerPivotingStrategy {
	FaerPivotingStrategy_Partial = 0,
	FaerPivotingStrategy_PartialDiag = 1,
	FaerPivotingStrategy_Rook = 2,
	FaerPivotingStrategy_RookDiag = 3,
	FaerPivotingStrategy_Full = 4
} FaerPivotingStrategy;
typedef struct FaerLbltParams { FaerPivotingStrategy pivoting; size_t par_threshold; size_t block_size; } FaerLbltParams;
typedef enum FaerLbltStatus_Tag { FaerLbltStatus_Ok = 0, FaerLbltStatus_Unknown = 1 } FaerLbltStatus_Tag;
typedef struct FaerLbltStatus {
	FaerLbltStatus_Tag tag;
	union { struct { size_t transposition_count; } ok; };
} FaerLbltStatus;
/* Cholesky with diagonal pivoting: faer.h:178-180, :432-453, lib.rs:559-571, :656-659 (cholesky/llt_pivoting/factor.rs:5-35) */
typedef struct FaerPivLltParams { size_t block_size; } FaerPivLltParams;
typedef enum FaerPivLltStatus_Tag { FaerPivLltStatus_Ok = 0, FaerPivLltStatus_NonPositivePivot = 1, FaerPivLltStatus_Unknown = 2 } FaerPivLltStatus_Tag;
typedef struct FaerPivLltStatus {
	FaerPivLltStatus_Tag tag;
	union {
		struct { size_t rank; size_t transposition_count; } ok;
		struct { size_t index; } non_positive_pivot;
	};
} FaerPivLltStatus;
/* faer-ffi/src/lib.rs:796-801; pointers to a real scalar of the matrix dtype (HOST memory), NULL == 0 */
typedef struct FaerLltRegularization { const void *dynamic_regularization_delta; const void *dynamic_regularization_epsilon; } FaerLltRegularization;
/* lib.rs:820-828: signs is a slice of i8 (HOST memory, `dim` entries) or a null ptr */
typedef struct FaerLdltRegularization { const void *dynamic_regularization_delta; const void *dynamic_regularization_epsilon; FaerSliceMut dynamic_regularization_signs; } FaerLdltRegularization;

/* ---------------------------------------------------------------------------------------------
 * 1. INNER boundary -- replaces private_gemm_x86::gemm (call sites above).
 * --------------------------------------------------------------------------------------------- */
typedef enum FaerHipDType { FaerHipDType_F32 = 0, FaerHipDType_F64 = 1, FaerHipDType_C32 = 2, FaerHipDType_C64 = 3 } FaerHipDType;
typedef enum FaerHipIType { FaerHipIType_U32 = 0, FaerHipIType_U64 = 1 } FaerHipIType;
typedef enum FaerHipDstKind { FaerHipDstKind_Full = 0, FaerHipDstKind_Lower = 1, FaerHipDstKind_Upper = 2 } FaerHipDstKind;

/* dst[row_idx[i], col_idx[j]] (or dst[i,j] when the index arrays are NULL), restricted to the
 * Full / Lower (i>=j) / Upper (i<=j) part, <- [dst +] alpha * lhs * diag(diag) * rhs.
 * Accum_Replace never reads dst.  F32 / F64 and C32 / C64 (interleaved {re, im}; strides in complex elements, alpha points at
 * one {re, im}).  conj_lhs / conj_rhs conjugate the operand (the identity for real scalars).  For C32 / C64 row_idx, col_idx and
 * diag must be NULL: the call aborts with a message that says so.
 * n_threads is accepted for signature compatibility and ignored.  Thread safe. */
FAER_HIP_API void faer_hip_gemm(FaerHipDType dtype, FaerHipIType itype, size_t m, size_t n, size_t k,
                                void *dst, ptrdiff_t dst_rs, ptrdiff_t dst_cs,
                                const void *row_idx, const void *col_idx,
                                FaerHipDstKind dst_kind, FaerAccum accum,
                                const void *lhs, ptrdiff_t lhs_rs, ptrdiff_t lhs_cs, bool conj_lhs,
                                const void *diag, ptrdiff_t diag_stride,
                                const void *rhs, ptrdiff_t rhs_rs, ptrdiff_t rhs_cs, bool conj_rhs,
                                const void *alpha, size_t n_threads);

/* ---------------------------------------------------------------------------------------------
 * 2. OUTER boundary -- faer-ffi symbol-compatible entry points (f32 / f64; level 3 -- matmul, matmul_triangular and the
 *    four triangular solves --, the four triangular inverses and the partial-pivot LU with its two solves also c32 / c64,
 *    where the FaerConj argument of the solves is honoured).
 *    Each comment cites the Rust function in faer-ffi/src/lib.rs it replaces.
 * --------------------------------------------------------------------------------------------- */
/* A client that includes the reference's own faer-ffi/faer.h for these prototypes (tests/cabi_client/) defines
 * FAER_HIP_NO_FFI_PROTOTYPES before including this header and gets the types and the faer_hip_* functions only
 * (two declarations of one symbol with layout-identical but differently named struct types do not mix in C). */
#ifndef FAER_HIP_NO_FFI_PROTOTYPES
/* lib.rs:855-871  la::matmul::matmul */
FAER_HIP_API void libfaer_v0_23_matmul_f64(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_f32(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_c64(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_c32(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha, FaerPar par);
/* lib.rs:872-895  la::matmul::triangular::matmul */
FAER_HIP_API void libfaer_v0_23_matmul_triangular_f64(FaerMatMut C, FaerBlock C_block, FaerAccum accum, FaerMatRef A, FaerBlock A_block, FaerMatRef B, FaerBlock B_block, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_triangular_f32(FaerMatMut C, FaerBlock C_block, FaerAccum accum, FaerMatRef A, FaerBlock A_block, FaerMatRef B, FaerBlock B_block, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_triangular_c64(FaerMatMut C, FaerBlock C_block, FaerAccum accum, FaerMatRef A, FaerBlock A_block, FaerMatRef B, FaerBlock B_block, const void *alpha, FaerPar par);
FAER_HIP_API void libfaer_v0_23_matmul_triangular_c32(FaerMatMut C, FaerBlock C_block, FaerAccum accum, FaerMatRef A, FaerBlock A_block, FaerMatRef B, FaerBlock B_block, const void *alpha, FaerPar par);
/* lib.rs:896-937  la::triangular_solve::solve_{,unit_}{lower,upper}_triangular_in_place_with_conj */
FAER_HIP_API void libfaer_v0_23_solve_triangular_lower_in_place_f64(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_lower_in_place_f32(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_lower_in_place_c64(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_lower_in_place_c32(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_upper_in_place_f64(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_upper_in_place_f32(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_upper_in_place_c64(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_triangular_upper_in_place_c32(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_lower_in_place_f64(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_lower_in_place_f32(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_lower_in_place_c64(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_lower_in_place_c32(FaerMatRef L, FaerConj L_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_upper_in_place_f64(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_upper_in_place_f32(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_upper_in_place_c64(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
FAER_HIP_API void libfaer_v0_23_solve_unit_triangular_upper_in_place_c32(FaerMatRef U, FaerConj U_conj, FaerMatMut rhs, FaerPar par);
/* lib.rs:938-983  la::triangular_inverse::invert_{,unit_}{lower,upper}_triangular for c32 / c64 (ctrtri.hip; the f32 / f64 prototypes
 * are in section 2b).  Only the named triangle of T is read and of T_inv written; unit: neither diagonal is touched. */
FAER_HIP_API void libfaer_v0_23_inverse_triangular_lower_in_place_c64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_lower_in_place_c32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_upper_in_place_c64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_upper_in_place_c32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_lower_in_place_c64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_lower_in_place_c32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_upper_in_place_c64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_upper_in_place_c32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);

/* lib.rs:650-655 (cparams! getter)  Auto<T> for LltParams: {64, 128} (cholesky/ldlt/factor.rs:705-714) */
FAER_HIP_API FaerLltParams libfaer_v0_23_LltParams_f64(void);
FAER_HIP_API FaerLltParams libfaer_v0_23_LltParams_f32(void);
/* lib.rs:984-995  cholesky_in_place_scratch (cholesky/llt/factor.rs:58-66): dim scalars */
FAER_HIP_API FaerLayout libfaer_v0_23_llt_factor_in_place_scratch_f64(size_t dim, FaerPar par, FaerLltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_factor_in_place_scratch_f32(size_t dim, FaerPar par, FaerLltParams params);
/* lib.rs:996-1011  cholesky_in_place (cholesky/llt/factor.rs:67-97) */
FAER_HIP_API FaerLltStatus libfaer_v0_23_llt_factor_in_place_f64(FaerMatMut A, FaerLltRegularization regularization, FaerPar par, FaerMemAlloc mem, FaerLltParams params);
FAER_HIP_API FaerLltStatus libfaer_v0_23_llt_factor_in_place_f32(FaerMatMut A, FaerLltRegularization regularization, FaerPar par, FaerMemAlloc mem, FaerLltParams params);
/* lib.rs:1012-1040  llt::solve::solve_in_place_with_conj (cholesky/llt/solve.rs:12-35) */
FAER_HIP_API FaerLayout libfaer_v0_23_llt_solve_in_place_scratch_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_solve_in_place_scratch_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_llt_solve_in_place_f64(FaerMatRef L, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void libfaer_v0_23_llt_solve_in_place_f32(FaerMatRef L, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);

/* lib.rs:679-685  Auto<T> for PartialPivLuParams: {16, 64, 128*128} (lu/partial_pivoting/factor.rs:212-222) */
FAER_HIP_API FaerPartialPivLuParams libfaer_v0_23_PartialPivLuParams_f64(void);
FAER_HIP_API FaerPartialPivLuParams libfaer_v0_23_PartialPivLuParams_f32(void);
/* lib.rs:1952-1965  lu_in_place_scratch (lu/partial_pivoting/factor.rs:224-233): min(dim, block_size) indices.
 * NB the ffi passes (dim, block_size) as (nrows, ncols). */
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u32_f64(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u64_f64(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u32_f32(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u64_f32(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
/* lib.rs:1966-1984  lu_in_place (lu/partial_pivoting/factor.rs:234-295); perm_fwd[i] = source row of row i of P*A */
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u32_f64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u64_f64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u32_f32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u64_f32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
/* the same for c32 / c64 (cgetrf.hip): the pivot of a column is its first entry of largest abs1 = |re| + |im| (factor.rs:35-43) */
FAER_HIP_API FaerPartialPivLuParams libfaer_v0_23_PartialPivLuParams_c64(void);
FAER_HIP_API FaerPartialPivLuParams libfaer_v0_23_PartialPivLuParams_c32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u32_c64(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u64_c64(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u32_c32(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_u64_c32(size_t dim, size_t block_size, FaerPar par, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u32_c64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u64_c64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u32_c32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);
FAER_HIP_API FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_u64_c32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPartialPivLuParams params);

/* lib.rs:667-671  Auto<T> for QrParams: {48*48, 192*256} (qr/no_pivoting/factor.rs:127-136) */
FAER_HIP_API FaerQrParams libfaer_v0_23_QrParams_f64(void);
FAER_HIP_API FaerQrParams libfaer_v0_23_QrParams_f32(void);
/* lib.rs:1520-1527  recommended_block_size (qr/no_pivoting/factor.rs:91-116) */
FAER_HIP_API size_t libfaer_v0_23_qr_recommended_block_size_f64(size_t nrows, size_t ncols);
FAER_HIP_API size_t libfaer_v0_23_qr_recommended_block_size_f32(size_t nrows, size_t ncols);
/* lib.rs:1528-1543  qr_in_place_scratch (qr/no_pivoting/factor.rs:305-316): block_size x ncols scalars */
FAER_HIP_API FaerLayout libfaer_v0_23_qr_factor_in_place_scratch_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerQrParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_factor_in_place_scratch_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerQrParams params);
/* lib.rs:1544-1559  qr_in_place (qr/no_pivoting/factor.rs:258-301); Q_coeff is block_size x min(m,n) */
FAER_HIP_API FaerQrStatus libfaer_v0_23_qr_factor_in_place_f64(FaerMatMut A, FaerMatMut Q_coeff, FaerPar par, FaerMemAlloc mem, FaerQrParams params);
FAER_HIP_API FaerQrStatus libfaer_v0_23_qr_factor_in_place_f32(FaerMatMut A, FaerMatMut Q_coeff, FaerPar par, FaerMemAlloc mem, FaerQrParams params);
/* lib.rs:1423-1470  apply_block_householder_sequence_{,transpose_}on_the_left_in_place_with_conj (householder.rs:724-808) */
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_on_the_left_scratch_f64(size_t dim, size_t block_size, size_t rhs_ncols);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_on_the_left_scratch_f32(size_t dim, size_t block_size, size_t rhs_ncols);
FAER_HIP_API void libfaer_v0_23_apply_householder_on_the_left_f64(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj householder_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void libfaer_v0_23_apply_householder_on_the_left_f32(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj householder_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_left_scratch_f64(size_t dim, size_t block_size, size_t rhs_ncols);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_left_scratch_f32(size_t dim, size_t block_size, size_t rhs_ncols);
FAER_HIP_API void libfaer_v0_23_apply_householder_transpose_on_the_left_f64(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj householder_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void libfaer_v0_23_apply_householder_transpose_on_the_left_f32(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj householder_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);


/* lib.rs:1985-2056  lu::partial_pivoting::solve::{solve_in_place, solve_transpose_in_place}_with_conj
 * (lu/partial_pivoting/solve.rs:20-80): rhs <- A^-1 rhs = U^-1 L^-1 P rhs, resp. rhs <- A^-T rhs.
 * perm slices are HOST memory with `dim` entries (element count, see SURVEY.md section 8b caveat iii). */
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u32_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u32_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u32_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u32_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u64_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u64_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u64_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u64_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
/* the same for c32 / c64, where A_conj is honoured: op(A) X = rhs / op(A)^T X = rhs with op the identity or the conjugate (solve.rs:21-87) */
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u32_c64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u32_c64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u32_c64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u32_c64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u32_c32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u32_c32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u32_c32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u32_c32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u64_c64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u64_c64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u64_c64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u64_c64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_u64_c32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_in_place_u64_c32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_u64_c32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_u64_c32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
/* lib.rs:1560-1660  qr::no_pivoting::solve::{solve_in_place, solve_transpose_in_place, solve_lstsq_in_place}_with_conj
 * (qr/no_pivoting/solve.rs:38-175): rhs <- R^-1 Q^H rhs (square or least squares: the solution is the top
 * ncols rows of rhs), resp. rhs <- Q R^-T rhs. */
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_in_place_scratch_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_in_place_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_transpose_in_place_scratch_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_transpose_in_place_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_lstsq_in_place_scratch_f64(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_lstsq_in_place_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_in_place_scratch_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_in_place_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_transpose_in_place_scratch_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_transpose_in_place_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_solve_lstsq_in_place_scratch_f32(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_solve_lstsq_in_place_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);


/* ---- next scope row: L D L^T without pivoting ---------------------------------
 * lib.rs:1189-1217  ldlt::factor::cholesky_in_place (cholesky/ldlt/factor.rs:742-800): unit lower L strictly below
 * the diagonal of A, D on it; lib.rs:1218-1250  ldlt::solve::solve_in_place_with_conj (cholesky/ldlt/solve.rs:12-50) */
FAER_HIP_API FaerLdltParams libfaer_v0_23_LdltParams_f64(void);
FAER_HIP_API FaerLdltParams libfaer_v0_23_LdltParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_factor_in_place_scratch_f64(size_t dim, FaerPar par, FaerLdltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_factor_in_place_scratch_f32(size_t dim, FaerPar par, FaerLdltParams params);
FAER_HIP_API FaerLdltStatus libfaer_v0_23_ldlt_factor_in_place_f64(FaerMatMut A, FaerLdltRegularization regularization, FaerPar par, FaerMemAlloc mem, FaerLdltParams params);
FAER_HIP_API FaerLdltStatus libfaer_v0_23_ldlt_factor_in_place_f32(FaerMatMut A, FaerLdltRegularization regularization, FaerPar par, FaerMemAlloc mem, FaerLdltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_solve_in_place_scratch_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_solve_in_place_scratch_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_ldlt_solve_in_place_f64(FaerMatRef L, FaerVecRef D, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void libfaer_v0_23_ldlt_solve_in_place_f32(FaerMatRef L, FaerVecRef D, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);

/* lib.rs:2523-2543  get/set_global_parallelism (faer/src/lib.rs:1107-1150).  Stored and returned only:
 * the GPU backend has no host thread pool. */
FAER_HIP_API FaerPar libfaer_v0_23_get_global_par(void);
FAER_HIP_API void libfaer_v0_23_set_global_par(FaerPar par);

/* ---------------------------------------------------------------------------------------------
 * 2b. Triangular inverse, reconstruct / inverse of the factorizations, reflectors applied on the right
 *     (faer-ffi/src/lib.rs:938-983, :1039-1075, :1247-1288, :1661-1720, :2071-2124, :1471-1518; f32/f64 subset).
 *     Same argument lists as the reference; the `mem` scratch is accepted and ignored (device scratch is
 *     pooled inside the library).  Triangular outputs leave the other triangle of `out` untouched.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API void libfaer_v0_23_inverse_triangular_lower_in_place_f64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_upper_in_place_f64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_lower_in_place_f64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_upper_in_place_f64(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_reconstruct_scratch_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_llt_reconstruct_f64(FaerMatMut A, FaerMatRef L, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_inverse_scratch_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_llt_inverse_f64(FaerMatMut A_inv, FaerMatRef L, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_reconstruct_scratch_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_ldlt_reconstruct_f64(FaerMatMut A, FaerMatRef L, FaerVecRef D, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_inverse_scratch_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_ldlt_inverse_f64(FaerMatMut A_inv, FaerMatRef L, FaerVecRef D, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_reconstruct_scratch_u32_f64(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_reconstruct_u32_f64(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_inverse_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_inverse_u32_f64(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_reconstruct_scratch_u64_f64(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_reconstruct_u64_f64(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_inverse_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_inverse_u64_f64(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_reconstruct_scratch_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_reconstruct_f64(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_inverse_scratch_f64(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_inverse_f64(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_on_the_right_scratch_f64(size_t dim, size_t block_size, size_t rhs_nrows);
FAER_HIP_API void libfaer_v0_23_apply_householder_on_the_right_f64(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj conj, FaerMatMut matrix, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_right_scratch_f64(size_t dim, size_t block_size, size_t rhs_nrows);
FAER_HIP_API void libfaer_v0_23_apply_householder_transpose_on_the_right_f64(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj conj, FaerMatMut matrix, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_lower_in_place_f32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_triangular_upper_in_place_f32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_lower_in_place_f32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API void libfaer_v0_23_inverse_unit_triangular_upper_in_place_f32(FaerMatMut T_inv, FaerMatRef T, FaerPar par);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_reconstruct_scratch_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_llt_reconstruct_f32(FaerMatMut A, FaerMatRef L, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_llt_inverse_scratch_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_llt_inverse_f32(FaerMatMut A_inv, FaerMatRef L, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_reconstruct_scratch_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_ldlt_reconstruct_f32(FaerMatMut A, FaerMatRef L, FaerVecRef D, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_ldlt_inverse_scratch_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_ldlt_inverse_f32(FaerMatMut A_inv, FaerMatRef L, FaerVecRef D, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_reconstruct_scratch_u32_f32(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_reconstruct_u32_f32(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_inverse_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_inverse_u32_f32(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_reconstruct_scratch_u64_f32(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_reconstruct_u64_f32(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_partial_piv_lu_inverse_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_partial_piv_lu_inverse_u64_f32(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_reconstruct_scratch_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_reconstruct_f32(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_qr_inverse_scratch_f32(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_qr_inverse_f32(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_on_the_right_scratch_f32(size_t dim, size_t block_size, size_t rhs_nrows);
FAER_HIP_API void libfaer_v0_23_apply_householder_on_the_right_f32(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj conj, FaerMatMut matrix, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_right_scratch_f32(size_t dim, size_t block_size, size_t rhs_nrows);
FAER_HIP_API void libfaer_v0_23_apply_householder_transpose_on_the_right_f32(FaerMatRef householder_basis, FaerMatRef householder_factor, FaerConj conj, FaerMatMut matrix, FaerPar par, FaerMemAlloc mem);

/* ---------------------------------------------------------------------------------------------
 * 2c. LU with full pivoting (faer-ffi/src/lib.rs:2125-2260; lu/full_pivoting/factor.rs, solve.rs): a level-2,
 *     HBM-bound algorithm -- every step is one fused "rank-1 update + search of the next pivot" pass (csrc/fplu.hip).
 *     Permutation slices are HOST memory (nrows / ncols entries).
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerFullPivLuParams libfaer_v0_23_FullPivLuParams_f64(void);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_factor_in_place_scratch_u32_f64(size_t dim, size_t block_size, FaerPar par, FaerFullPivLuParams params);
FAER_HIP_API FaerFullPivLuStatus libfaer_v0_23_full_piv_lu_factor_in_place_u32_f64(FaerMatMut A, FaerSliceMut row_perm_fwd, FaerSliceMut row_perm_bwd, FaerSliceMut col_perm_fwd, FaerSliceMut col_perm_bwd, FaerPar par, FaerMemAlloc mem, FaerFullPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_in_place_u32_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_transpose_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_transpose_in_place_u32_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_factor_in_place_scratch_u64_f64(size_t dim, size_t block_size, FaerPar par, FaerFullPivLuParams params);
FAER_HIP_API FaerFullPivLuStatus libfaer_v0_23_full_piv_lu_factor_in_place_u64_f64(FaerMatMut A, FaerSliceMut row_perm_fwd, FaerSliceMut row_perm_bwd, FaerSliceMut col_perm_fwd, FaerSliceMut col_perm_bwd, FaerPar par, FaerMemAlloc mem, FaerFullPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_in_place_u64_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_transpose_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_transpose_in_place_u64_f64(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerFullPivLuParams libfaer_v0_23_FullPivLuParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_factor_in_place_scratch_u32_f32(size_t dim, size_t block_size, FaerPar par, FaerFullPivLuParams params);
FAER_HIP_API FaerFullPivLuStatus libfaer_v0_23_full_piv_lu_factor_in_place_u32_f32(FaerMatMut A, FaerSliceMut row_perm_fwd, FaerSliceMut row_perm_bwd, FaerSliceMut col_perm_fwd, FaerSliceMut col_perm_bwd, FaerPar par, FaerMemAlloc mem, FaerFullPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_in_place_u32_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_transpose_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_transpose_in_place_u32_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_factor_in_place_scratch_u64_f32(size_t dim, size_t block_size, FaerPar par, FaerFullPivLuParams params);
FAER_HIP_API FaerFullPivLuStatus libfaer_v0_23_full_piv_lu_factor_in_place_u64_f32(FaerMatMut A, FaerSliceMut row_perm_fwd, FaerSliceMut row_perm_bwd, FaerSliceMut col_perm_fwd, FaerSliceMut col_perm_bwd, FaerPar par, FaerMemAlloc mem, FaerFullPivLuParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_in_place_u64_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_solve_transpose_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_solve_transpose_in_place_u64_f32(FaerMatRef L, FaerMatRef U, FaerConj A_conj, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);

/* ---------------------------------------------------------------------------------------------
 * 2d. QR with column pivoting (faer-ffi/src/lib.rs:1721-1876; qr/col_pivoting/factor.rs, solve.rs): HBM-bound;
 *     delayed rank-1 updates fused with the next step's dot products, down-dated column norms with the reference's
 *     recomputation rule (csrc/colpiv_qr.hip, colpiv_qr_dev).  Permutation slices are HOST memory (ncols entries).
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerColPivQrParams libfaer_v0_23_ColPivQrParams_f64(void);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_factor_in_place_scratch_u32_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerColPivQrParams params);
FAER_HIP_API FaerColPivQrStatus libfaer_v0_23_colpiv_qr_factor_in_place_u32_f64(FaerMatMut A, FaerMatMut Q_coeff, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerColPivQrParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_in_place_scratch_u32_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_in_place_u32_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_transpose_in_place_scratch_u32_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_transpose_in_place_u32_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_scratch_u32_f64(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_u32_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_factor_in_place_scratch_u64_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerColPivQrParams params);
FAER_HIP_API FaerColPivQrStatus libfaer_v0_23_colpiv_qr_factor_in_place_u64_f64(FaerMatMut A, FaerMatMut Q_coeff, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerColPivQrParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_in_place_scratch_u64_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_in_place_u64_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_transpose_in_place_scratch_u64_f64(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_transpose_in_place_u64_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_scratch_u64_f64(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_u64_f64(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerColPivQrParams libfaer_v0_23_ColPivQrParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_factor_in_place_scratch_u32_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerColPivQrParams params);
FAER_HIP_API FaerColPivQrStatus libfaer_v0_23_colpiv_qr_factor_in_place_u32_f32(FaerMatMut A, FaerMatMut Q_coeff, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerColPivQrParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_in_place_scratch_u32_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_in_place_u32_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_transpose_in_place_scratch_u32_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_transpose_in_place_u32_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_scratch_u32_f32(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_u32_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_factor_in_place_scratch_u64_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par, FaerColPivQrParams params);
FAER_HIP_API FaerColPivQrStatus libfaer_v0_23_colpiv_qr_factor_in_place_u64_f32(FaerMatMut A, FaerMatMut Q_coeff, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerColPivQrParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_in_place_scratch_u64_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_in_place_u64_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_transpose_in_place_scratch_u64_f32(size_t dim, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_transpose_in_place_u64_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_scratch_u64_f32(size_t nrows, size_t ncols, size_t block_size, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_u64_f32(FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);

/* reconstruct / inverse of the pivoted factorizations (faer-ffi/src/lib.rs:1877-1950, :2246-2330) */
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_reconstruct_scratch_u32_f64(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_reconstruct_u32_f64(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_inverse_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_inverse_u32_f64(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_reconstruct_scratch_u32_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_reconstruct_u32_f64(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_inverse_scratch_u32_f64(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_inverse_u32_f64(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_reconstruct_scratch_u64_f64(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_reconstruct_u64_f64(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_inverse_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_inverse_u64_f64(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_reconstruct_scratch_u64_f64(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_reconstruct_u64_f64(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_inverse_scratch_u64_f64(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_inverse_u64_f64(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_reconstruct_scratch_u32_f32(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_reconstruct_u32_f32(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_inverse_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_inverse_u32_f32(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_reconstruct_scratch_u32_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_reconstruct_u32_f32(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_inverse_scratch_u32_f32(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_inverse_u32_f32(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_reconstruct_scratch_u64_f32(size_t nrows, size_t ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_reconstruct_u64_f32(FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_full_piv_lu_inverse_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_full_piv_lu_inverse_u64_f32(FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef row_perm_fwd, FaerSliceRef row_perm_bwd, FaerSliceRef col_perm_fwd, FaerSliceRef col_perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_reconstruct_scratch_u64_f32(size_t nrows, size_t ncols, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_reconstruct_u64_f32(FaerMatMut A, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_colpiv_qr_inverse_scratch_u64_f32(size_t dim, size_t block_size, FaerPar par);
FAER_HIP_API void libfaer_v0_23_colpiv_qr_inverse_u64_f32(FaerMatMut A_inv, FaerMatRef Q_basis, FaerMatRef Q_coeff, FaerMatRef R, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
/* ---------------------------------------------------------------------------------------------
 * 2e. Self-adjoint eigendecomposition (faer-ffi/src/lib.rs:2368-2400; evd/mod.rs:270-425): A = U diag(S) U^H.
 *     A (n x n): only its lower triangle is read, A is never written.  S (n entries) receives the eigenvalues in
 *     ascending order.  U.ncols == 0: no eigenvectors; otherwise U is n x n and column j is the unit eigenvector of
 *     S[j].  Tridiagonalization (csrc/condense.hip), divide and conquer on the tridiagonal with QR-iteration leaves
 *     (csrc/evd.hip), block Householder back-transform.  Leaves hold at most min(max(recursion_threshold, 4), 64) rows:
 *     a larger threshold is clamped to 64 (the decomposition is the same up to rounding).  par, mem and
 *     params.tridiag are accepted and ignored.  NoConvergence: a non-finite entry in the tridiagonal form, or a leaf
 *     over the reference's iteration cap.  Host or device operands, any strides.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerTridiagParams libfaer_v0_23_TridiagParams_f64(void);
FAER_HIP_API FaerTridiagParams libfaer_v0_23_TridiagParams_f32(void);
FAER_HIP_API FaerSelfAdjointEvdParams libfaer_v0_23_SelfAdjointEvdParams_f64(void);
FAER_HIP_API FaerSelfAdjointEvdParams libfaer_v0_23_SelfAdjointEvdParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_self_adjoint_evd_scratch_f64(size_t dim, FaerComputeEigenvectors compute_U, FaerPar par, FaerSelfAdjointEvdParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_self_adjoint_evd_scratch_f32(size_t dim, FaerComputeEigenvectors compute_U, FaerPar par, FaerSelfAdjointEvdParams params);
FAER_HIP_API FaerEvdStatus libfaer_v0_23_self_adjoint_evd_f64(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerPar par, FaerMemAlloc mem, FaerSelfAdjointEvdParams params);
FAER_HIP_API FaerEvdStatus libfaer_v0_23_self_adjoint_evd_f32(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerPar par, FaerMemAlloc mem, FaerSelfAdjointEvdParams params);
/* ---------------------------------------------------------------------------------------------
 * 2f. Singular value decomposition (faer-ffi/src/lib.rs:2327-2366; svd/mod.rs:530-671): A = U[:, :k] diag(S) V[:, :k]^T,
 *     k = min(nrows, ncols).  A (m x n) is never written.  S (k entries) receives the singular values, nonnegative and
 *     nonincreasing.  U.ncols == 0: no left vectors; otherwise U is m x k (thin) or m x m (full).  V.ncols == 0: no right
 *     vectors; otherwise V is n x k or n x n.  k == 0: S is empty and a requested m x m U (n x n V for m == 0) receives
 *     the identity.  A wide matrix runs as its transpose; a tall one with m / n > qr_ratio_threshold goes through a QR
 *     factorization first.  Bidiagonalization (csrc/condense.hip), divide and conquer on the bidiagonal with
 *     QR-iteration leaves (csrc/svd.hip), two block Householder back-transforms.  Leaves hold at most
 *     min(max(recursion_threshold, 4), 64) entries: a larger threshold is clamped to 64.  par, mem, params.bidiag and
 *     params.qr.par_threshold are accepted and ignored.  NoConvergence: a non-finite entry in the bidiagonal form, or a
 *     leaf over the reference's iteration cap.  Host or device operands, any strides; only the addressed elements are
 *     written.  The scratch query needs no device.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerBidiagParams libfaer_v0_23_BidiagParams_f64(void);
FAER_HIP_API FaerBidiagParams libfaer_v0_23_BidiagParams_f32(void);
FAER_HIP_API FaerSvdParams libfaer_v0_23_SvdParams_f64(void);
FAER_HIP_API FaerSvdParams libfaer_v0_23_SvdParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_svd_scratch_f64(size_t nrows, size_t ncols, FaerComputeSvdVectors compute_U, FaerComputeSvdVectors compute_V, FaerPar par, FaerSvdParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_svd_scratch_f32(size_t nrows, size_t ncols, FaerComputeSvdVectors compute_U, FaerComputeSvdVectors compute_V, FaerPar par, FaerSvdParams params);
FAER_HIP_API FaerSvdStatus libfaer_v0_23_svd_f64(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerMatMut V, FaerPar par, FaerMemAlloc mem, FaerSvdParams params);
FAER_HIP_API FaerSvdStatus libfaer_v0_23_svd_f32(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerMatMut V, FaerPar par, FaerMemAlloc mem, FaerSvdParams params);
/* ---------------------------------------------------------------------------------------------
 * 2g. LBLT: Bunch-Kaufman factorization of a symmetric indefinite matrix (faer-ffi/src/lib.rs:1288-1421;
 *     cholesky/bunch_kaufman/factor.rs, solve.rs, reconstruct.rs, inverse.rs): P A P^T = L B L^T, B block diagonal with
 *     1 x 1 and 2 x 2 blocks.  Only the LOWER triangle of A is read or written; the strict upper triangle is never touched.
 *     On return the strict lower triangle holds the unit lower L, the diagonal holds the diagonal of B, subdiag[j] =
 *     B[j+1, j] for a 2 x 2 block starting at j (then subdiag[j+1] == 0 and A[j+1, j] is stored as 0) and 0 for a 1 x 1
 *     block.  perm_fwd[i] = source index of row i of P A P^T, perm_bwd its inverse (HOST memory, dim entries);
 *     transposition_count = number of positions whose pivot index differs from the position.  Pivoting strategies
 *     Partial, PartialDiag (the default), Rook and RookDiag follow the reference's decision tree, ties of every arg-max
 *     going to the lowest index.  A value of params.pivoting outside the enum aborts with a message naming it (the
 *     boundary's convention for unsupported input); faer_hip_lblt_pivoting_supported (section 3) asks instead.
 *     params.block_size and par_threshold are
 *     hints and ignored: the GPU factors panels of 64 columns by the lazily updated W-panel algorithm and the last <= 64
 *     rows in one LDS-resident workgroup (csrc/lblt.hip); the pivot sequence does not depend on the blocking in exact
 *     arithmetic.
 *     Full (factor.rs:264-429, lblt_full_piv) is a level-2 algorithm of its own: the lower triangle is multiplied by the
 *     reciprocal of its largest magnitude; every step takes the first largest diagonal entry of the trailing matrix as a
 *     1 x 1 pivot if its square is >= ((1 + sqrt 17) / 8)^2 times the largest squared off-diagonal entry (ties: lowest
 *     column, then lowest row), else that off-diagonal entry as a 2 x 2 pivot; once the trailing off-diagonal is zero the
 *     remaining diagonal is only ordered by decreasing magnitude; at the end the diagonal and subdiag are multiplied by
 *     the scale (L has none).  Three deliberate deviations from the reference: (1) the reference takes the largest
 *     magnitude of the whole matrix, scales the whole matrix and leaves its strict upper triangle scaled; here the strict
 *     upper triangle is neither read nor written, as for every strategy -- for a symmetric input the lower triangle,
 *     subdiag and the permutations are the same; (2) for the zero matrix the reference forms 0 * inf; here both scalings
 *     are skipped and the result is the input unchanged, zero subdiag, identity permutation, count 0; (3) for non-finite
 *     input, and for a scale whose reciprocal overflows, the call returns Ok, terminates and writes only inside the lower
 *     triangle; nothing is promised about the values.
 *     solve / reconstruct / inverse take L and the strided `diag` and `subdiag` vectors as the factorization
 *     leaves them; reconstruct writes the lower triangle of A only, inverse the whole of A_inv.  Host or device operands,
 *     any strides; par, mem and A_conj are accepted and ignored.  The scratch queries need no device.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerLbltParams libfaer_v0_23_LbltParams_f64(void);
FAER_HIP_API FaerLbltParams libfaer_v0_23_LbltParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_factor_in_place_scratch_u32_f64(size_t dim, FaerPar par, FaerLbltParams params);
FAER_HIP_API FaerLbltStatus libfaer_v0_23_lblt_factor_in_place_u32_f64(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerLbltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_solve_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_solve_in_place_u32_f64(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_reconstruct_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_reconstruct_u32_f64(FaerMatMut A, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_inverse_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_inverse_u32_f64(FaerMatMut A_inv, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_factor_in_place_scratch_u32_f32(size_t dim, FaerPar par, FaerLbltParams params);
FAER_HIP_API FaerLbltStatus libfaer_v0_23_lblt_factor_in_place_u32_f32(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerLbltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_solve_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_solve_in_place_u32_f32(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_reconstruct_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_reconstruct_u32_f32(FaerMatMut A, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_inverse_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_inverse_u32_f32(FaerMatMut A_inv, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_factor_in_place_scratch_u64_f64(size_t dim, FaerPar par, FaerLbltParams params);
FAER_HIP_API FaerLbltStatus libfaer_v0_23_lblt_factor_in_place_u64_f64(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerLbltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_solve_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_solve_in_place_u64_f64(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_reconstruct_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_reconstruct_u64_f64(FaerMatMut A, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_inverse_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_inverse_u64_f64(FaerMatMut A_inv, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_factor_in_place_scratch_u64_f32(size_t dim, FaerPar par, FaerLbltParams params);
FAER_HIP_API FaerLbltStatus libfaer_v0_23_lblt_factor_in_place_u64_f32(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerLbltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_solve_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_solve_in_place_u64_f32(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerConj A_conj, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_reconstruct_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_reconstruct_u64_f32(FaerMatMut A, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_lblt_inverse_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_lblt_inverse_u64_f32(FaerMatMut A_inv, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
/* ---------------------------------------------------------------------------------------------
 * 2h. PIV_LLT: Cholesky factorization with diagonal pivoting of a symmetric positive semidefinite matrix (faer-ffi/src/lib.rs:
 *     1076-1188; cholesky/llt_pivoting/factor.rs, solve.rs, reconstruct.rs, inverse.rs; LAPACK's pstrf): P A P^T = L L^T.  Only the
 *     LOWER triangle of A is read or written; the strict upper triangle is never touched.  perm_fwd[i] = source index of row i of
 *     P A P^T, perm_bwd its inverse (HOST memory, dim entries).  Every step takes the first strict maximum of the updated diagonal
 *     as its pivot (ties: the lowest index); a negative or NaN entry of the diagonal of A returns NonPositivePivot{0} with A
 *     unmodified, a NaN in the updated diagonal at step j NonPositivePivot{j}.  From step 1 on a pivot below tol = eps * dim *
 *     max diag(A) ends the factorization with Ok{rank = j}: A[j, j] receives that pivot, columns < rank of L, both permutations and
 *     transposition_count (the number of steps whose pivot differs from the step) are defined, the rest of the lower triangle from
 *     column rank on is unspecified.  As in the reference the test is not made at step 0: the zero matrix of order >= 2 returns
 *     NonPositivePivot{1}, of order 1 Ok{rank 1}.  params.block_size is a hint and ignored: the GPU factors lazily updated panels of
 *     64 columns, two launches per column and no host synchronisation inside a panel, and the last <= 64 rows in one LDS-resident
 *     workgroup (csrc/piv_llt.hip); the pivot sequence does not depend on the blocking in exact arithmetic.  solve / reconstruct /
 *     inverse take L as a full-rank factorization leaves it; reconstruct and inverse write the lower triangle of their output only.
 *     Host or device operands, any strides; par, mem and A_conj are accepted and ignored.  The scratch queries need no device.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API FaerPivLltParams libfaer_v0_23_PivLltParams_f64(void);
FAER_HIP_API FaerPivLltParams libfaer_v0_23_PivLltParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_factor_in_place_scratch_u32_f64(size_t dim, FaerPar par, FaerPivLltParams params);
FAER_HIP_API FaerPivLltStatus libfaer_v0_23_piv_llt_factor_in_place_u32_f64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPivLltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_solve_in_place_scratch_u32_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_solve_in_place_u32_f64(FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_reconstruct_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_reconstruct_u32_f64(FaerMatMut A, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_inverse_scratch_u32_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_inverse_u32_f64(FaerMatMut A_inv, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_factor_in_place_scratch_u32_f32(size_t dim, FaerPar par, FaerPivLltParams params);
FAER_HIP_API FaerPivLltStatus libfaer_v0_23_piv_llt_factor_in_place_u32_f32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPivLltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_solve_in_place_scratch_u32_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_solve_in_place_u32_f32(FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_reconstruct_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_reconstruct_u32_f32(FaerMatMut A, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_inverse_scratch_u32_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_inverse_u32_f32(FaerMatMut A_inv, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_factor_in_place_scratch_u64_f64(size_t dim, FaerPar par, FaerPivLltParams params);
FAER_HIP_API FaerPivLltStatus libfaer_v0_23_piv_llt_factor_in_place_u64_f64(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPivLltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_solve_in_place_scratch_u64_f64(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_solve_in_place_u64_f64(FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_reconstruct_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_reconstruct_u64_f64(FaerMatMut A, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_inverse_scratch_u64_f64(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_inverse_u64_f64(FaerMatMut A_inv, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_factor_in_place_scratch_u64_f32(size_t dim, FaerPar par, FaerPivLltParams params);
FAER_HIP_API FaerPivLltStatus libfaer_v0_23_piv_llt_factor_in_place_u64_f32(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerPivLltParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_solve_in_place_scratch_u64_f32(size_t dim, size_t rhs_ncols, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_solve_in_place_u64_f32(FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerConj A_conj, FaerMatMut rhs, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_reconstruct_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_reconstruct_u64_f32(FaerMatMut A, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout libfaer_v0_23_piv_llt_inverse_scratch_u64_f32(size_t dim, FaerPar par);
FAER_HIP_API void libfaer_v0_23_piv_llt_inverse_u64_f32(FaerMatMut A_inv, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem);


/* ---------------------------------------------------------------------------------------------
 * 2i. General (nonsymmetric) real eigendecomposition (faer-ffi/src/lib.rs:2402-2457; evd/mod.rs:960-1246, evd_real).
 *     A (n x n) is never written.  S / S_im (n entries each) receive the real / imaginary parts of the eigenvalues.
 *     UL.ncols == 0 / UR.ncols == 0: left / right eigenvectors not wanted; otherwise n x n.  A real eigenvalue
 *     (S_im[i] == 0) has its eigenvector in column i.  A complex pair sits at (i, i + 1) with S_im[i] == -S_im[i + 1] != 0,
 *     S_im[i] > 0: column i holds the real and column i + 1 the imaginary part of the eigenvector of S[i] + i S_im[i]; for UL
 *     the relation is ul^H A = s ul^H (evd/mod.rs:1325-1352).  Vectors are not normalised (as in the reference).
 *     Hessenberg reduction (csrc/condense.hip), real Schur form by multishift QR sweeps with LDS-resident windows and
 *     double-shift leaves, back substitution on the quasi-triangular factor, two triangular products (csrc/schur.hip).
 *     Honoured: params.schur.recommended_shift_count (called on the host once per sweep with (n, active block size); the
 *     result is rounded down to an even number and clamped to 2 .. min(active - 1, 2 * (W / 6)), W = 96 for f64 and 128 for
 *     f32, what a bulge chain in one window holds).  Accepted and unused: par, mem, params.hessenberg,
 *     params.schur.recommended_deflation_window and nibble_threshold (no aggressive early deflation: the classical
 *     small-subdiagonal test only), params.schur.blocking_threshold (an active block of at most W rows is finished by the
 *     leaf kernel) and params.evd_from_schur.recursion_threshold (every eigenvector is one column-oriented solve).
 *     NoConvergence: a non-finite entry of A (checked on the device before anything else), or the iteration cap
 *     30 max(10, n) of sweeps / of a leaf.  Range: the eigenvalues are right for entries anywhere in the floating-point range
 *     (the Schur stage forms no squares of entries).  The eigenvectors are not: the closed-form solves of the 2 x 2 diagonal
 *     blocks square entries of the Schur form (a * a - b * c), as the reference's do (evd/mod.rs:670-881), so with entries
 *     beyond the square root of the largest or smallest number a call that asks for vectors may return Ok with vectors that
 *     hold Inf, NaN or zeros.  Scale such a matrix by a power of two first; the eigenvalues scale with it, the vectors do not
 *     change.  Violated shape preconditions abort.  Host or device operands, any strides, on the
 *     caller's stream; the call returns after its last kernel has finished.  The scratch query needs no device.
 *     faer_hip_default_recommended_shift_count / _deflation_window are the reference's defaults (evd/schur/mod.rs:59-107),
 *     the two function pointers of libfaer_v0_23_SchurParams_*.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API size_t faer_hip_default_recommended_shift_count(size_t matrix_dimension, size_t active_block_dimension);
FAER_HIP_API size_t faer_hip_default_recommended_deflation_window(size_t matrix_dimension, size_t active_block_dimension);
FAER_HIP_API FaerHessenbergParams libfaer_v0_23_HessenbergParams_f64(void);
FAER_HIP_API FaerHessenbergParams libfaer_v0_23_HessenbergParams_f32(void);
FAER_HIP_API FaerSchurParams libfaer_v0_23_SchurParams_f64(void);
FAER_HIP_API FaerSchurParams libfaer_v0_23_SchurParams_f32(void);
FAER_HIP_API FaerEvdFromSchurParams libfaer_v0_23_EvdFromSchurParams_f64(void);
FAER_HIP_API FaerEvdFromSchurParams libfaer_v0_23_EvdFromSchurParams_f32(void);
FAER_HIP_API FaerEvdParams libfaer_v0_23_EvdParams_f64(void);
FAER_HIP_API FaerEvdParams libfaer_v0_23_EvdParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_evd_scratch_f64(size_t dim, FaerComputeEigenvectors compute_left, FaerComputeEigenvectors compute_right, FaerPar par, FaerEvdParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_evd_scratch_f32(size_t dim, FaerComputeEigenvectors compute_left, FaerComputeEigenvectors compute_right, FaerPar par, FaerEvdParams params);
FAER_HIP_API FaerEvdStatus libfaer_v0_23_evd_f64(FaerMatRef A, FaerMatMut UL, FaerMatMut UR, FaerVecMut S, FaerVecMut S_im, FaerPar par, FaerMemAlloc mem, FaerEvdParams params);
FAER_HIP_API FaerEvdStatus libfaer_v0_23_evd_f32(FaerMatRef A, FaerMatMut UL, FaerMatMut UR, FaerVecMut S, FaerVecMut S_im, FaerPar par, FaerMemAlloc mem, FaerEvdParams params);
/* ---------------------------------------------------------------------------------------------
 * 2j. Generalized real eigendecomposition (faer-ffi/src/lib.rs:2459-2520; gevd/mod.rs:130-320, gevd_real) of the pair (A, B).
 *     Eigenvalue i is (alpha[i] + i alpha_im[i]) / beta[i]; beta[i] >= 0, and beta[i] == 0 is an infinite eigenvalue.  UL / UR
 *     with no columns: not wanted.  Vectors use the packed layout of evd: a real eigenvalue takes column i, a conjugate pair at
 *     (i, i + 1) takes real part, then imaginary part; ur: beta A x = alpha B x, ul: beta y^H A = alpha y^H B.  Columns are not
 *     normalised.  A non-finite entry of A or B fills alpha, alpha_im, beta and the wanted vectors with NaN and returns
 *     NoConvergence.  The reference leaves A and B unspecified after the call; this library works on device copies and does
 *     not write them.  Operands may be host or device memory with arbitrary element strides; the call runs on the caller's
 *     stream and takes all its device memory from one arena.
 *     Path: QR of B, Hessenberg-triangular reduction by rotations in one workgroup, multishift QZ sweeps in LDS windows of edge
 *     faer_hip_gevd_window_edge with off-window products on the GEMM and an LDS-resident leaf for blocks up to that edge
 *     (csrc/qz.hip, csrc/qz_core.h), eigenvectors one workgroup per eigenvalue.  schur.recommended_shift_count is called once per
 *     sweep and clamped to [2, twice the bulges a window carries], even.  Accepted and unused: hessenberg.block_size and
 *     .blocking_threshold (the blocked reduction), the other fields of schur (no aggressive early deflation yet),
 *     evd_from_schur.  `par` and `mem` are ignored.
 * --------------------------------------------------------------------------------------------- */
FAER_HIP_API size_t faer_hip_default_relative_cost_estimate_of_shift_chase_to_matmul(size_t matrix_dimension, size_t active_block_dimension);
FAER_HIP_API FaerGeneralizedHessenbergParams libfaer_v0_23_GeneralizedHessenbergParams_f64(void);
FAER_HIP_API FaerGeneralizedHessenbergParams libfaer_v0_23_GeneralizedHessenbergParams_f32(void);
FAER_HIP_API FaerGeneralizedSchurParams libfaer_v0_23_GeneralizedSchurParams_f64(void);
FAER_HIP_API FaerGeneralizedSchurParams libfaer_v0_23_GeneralizedSchurParams_f32(void);
FAER_HIP_API FaerGevdParams libfaer_v0_23_GevdParams_f64(void);
FAER_HIP_API FaerGevdParams libfaer_v0_23_GevdParams_f32(void);
FAER_HIP_API FaerLayout libfaer_v0_23_generalized_evd_scratch_f64(size_t dim, FaerComputeEigenvectors compute_left, FaerComputeEigenvectors compute_right, FaerPar par, FaerGevdParams params);
FAER_HIP_API FaerLayout libfaer_v0_23_generalized_evd_scratch_f32(size_t dim, FaerComputeEigenvectors compute_left, FaerComputeEigenvectors compute_right, FaerPar par, FaerGevdParams params);
FAER_HIP_API FaerGevdStatus libfaer_v0_23_generalized_evd_f64(FaerMatMut A, FaerMatMut B, FaerMatMut UL, FaerMatMut UR, FaerVecMut alpha, FaerVecMut alpha_im, FaerVecMut beta, FaerPar par, FaerMemAlloc mem, FaerGevdParams params);
FAER_HIP_API FaerGevdStatus libfaer_v0_23_generalized_evd_f32(FaerMatMut A, FaerMatMut B, FaerMatMut UL, FaerMatMut UR, FaerVecMut alpha, FaerVecMut alpha_im, FaerVecMut beta, FaerPar par, FaerMemAlloc mem, FaerGevdParams params);
#endif /* FAER_HIP_NO_FFI_PROTOTYPES */
/* debug / measurement: {sweeps, window steps, leaf launches, state read-backs} of the calling thread's last evd; the window edge W */
FAER_HIP_API void faer_hip_debug_evd_last_counts(long out[4]);
FAER_HIP_API size_t faer_hip_evd_window_edge(FaerHipDType dtype);
/* {multishift sweeps, window steps, leaf launches, state read-backs, infinite eigenvalues deflated} of the calling thread's last
 * generalized_evd; the window edge W (64 for f64, 96 for f32) */
FAER_HIP_API void faer_hip_debug_gevd_last_counts(long out[5]);
FAER_HIP_API size_t faer_hip_gevd_window_edge(FaerHipDType dtype);
/* ---------------------------------------------------------------------------------------------
 * 3. Runtime control (new: the reference has no device).
 * --------------------------------------------------------------------------------------------- */
/* Library version / build target string, e.g. "faer_hip 0.1 gfx950". Never NULL. */
FAER_HIP_API const char *faer_hip_version(void);
/* Number of usable gfx950 devices (0 when none: compute entry points will abort). */
FAER_HIP_API int faer_hip_device_count(void);
/* Binds the calling thread to `device` (hipSetDevice). */
FAER_HIP_API void faer_hip_set_device(int device);
/* All work of the calling thread is enqueued on `hip_stream` (a hipStream_t; NULL = the null stream).
 * Lets a host framework (e.g. torch's current stream) order our kernels with its own. */
FAER_HIP_API void faer_hip_set_stream(void *hip_stream);
FAER_HIP_API void *faer_hip_get_stream(void);
/* Blocks until all work enqueued on the calling thread's stream is done. */
FAER_HIP_API void faer_hip_synchronize(void);
/* Releases the calling thread's internal look-ahead streams and events (they are re-created on demand).
 * Call before unloading the library or at process exit. */
FAER_HIP_API void faer_hip_shutdown(void);
/* 1 if libfaer_v0_23_lblt_factor_in_place_* runs `pivoting` (the five values of FaerPivotingStrategy), 0 for any other value, which
 * that entry point would abort on.  Makes no GPU call and creates no context. */
FAER_HIP_API int faer_hip_lblt_pivoting_supported(FaerPivotingStrategy pivoting);
/* Device memory helpers for C clients without another allocator. */
FAER_HIP_API void *faer_hip_malloc(size_t bytes);
FAER_HIP_API void faer_hip_free(void *ptr);
FAER_HIP_API void faer_hip_memcpy_h2d(void *dst_device, const void *src_host, size_t bytes);
FAER_HIP_API void faer_hip_memcpy_d2h(void *dst_host, const void *src_device, size_t bytes);
/* Tuning knob used by bench.py / tests: the GEMM tile variant of the calling thread.  0 = auto (the rules of the dispatch),
 * 1 / 2 = force the pipelined 128 x 128 / 64 x 64 tile, 3 = force the 128 x 256 tile wherever it can run (plain full and square
 * lower products), 5 = auto without the 128 x 256 tile, 6 = 128 x 128 tiles for every short-wide / tall-narrow full product with
 * K >= 2048 (what the QR block applications ask for themselves), 11 / 12 = the non-pipelined kernel on 128 x 128 / 64 x 64
 * tiles.  Structured operands and diag scaling always run the 64 x 64 kernel made for them. */
FAER_HIP_API void faer_hip_set_gemm_variant(int variant);
/* Host-side dispatch of the dense GEMM, callable without a GPU (unit tests): what gemm_dev decides for a product that has not
 * left for a level-2 kernel (K >= 1; rank-1, matrix-vector and skinny shapes are decided by those kernels themselves).
 * problem[24] = {m, n, k, bytes per element (4 / 8), dst kind (FaerHipDstKind), add (0 / 1), alpha (1: +1, -1: -1, 0: another value),
 * dst row stride, dst col stride, lhs row, lhs col, rhs row, rhs col stride (elements), index arrays given (0 / 1), diag given (0 / 1),
 * lhs FaerBlock, rhs FaerBlock, k_trim, tri_skip, stair_nb, stair_gap, stair_row0, prefer_big_tiles (0 / 1), variant (see
 * faer_hip_set_gemm_variant)}, as the caller passes the product (before any transposition).
 * plan[16] = {transposed (the product runs on dst^T; tile counts and loaders below refer to that orientation), tile kind (0 the 64 x 64
 * kernel for structured operands / diag, 1 / 2 / 3 pipelined 64 x 64 / 128 x 128 / 128 x 256, 4 / 5 non-pipelined 64 x 64 / 128 x 128),
 * tri_skip split into two plain products (0 / 1; then only the loaders and the routes are set besides), lhs K-major loader, rhs K-major loader, tile rows, tile
 * columns, tiles along m, tiles along n, triangular tile enumeration (0 / 1), first tile of it, K splits, K per split, fused epilogue
 * (0 none, 1 Replace, 2 / 3 Add with alpha +1 / -1), profile class (0 big pipelined tile, -1 none), routes (bit r: FaerHipRoute r counts)}.
 * Returns 0; 1 if the library refuses the product (it would abort with *refusal, a static string; `refusal` may be NULL); -1 if
 * `problem` is not a dense product (a dimension < 1 or >= 2^31, an element size other than 4 / 8, codes out of range). */
FAER_HIP_API int faer_hip_debug_gemm_plan(const long long problem[24], int plan[16], const char **refusal);
/* Debugging aid.  `which`: 0 = the caller's stream, 1 / 2 = the internal bulk / panel look-ahead stream; writes
 * {XCC id, HW_ID} of the CU each of `nblocks` probe workgroups ran on (2 * nblocks words of host memory). */
FAER_HIP_API void faer_hip_debug_stream_xcc(int which, int nblocks, unsigned *out_host);
/* Host-side planning logic of the drivers, callable without a GPU (unit tests): the look-ahead panel starts of the
 * blocked Cholesky (last entry = start of the sequential tail; returns the number of entries) and the leaf width
 * the cooperative LU panel kernel picks for `nrows` rows when `resident_workgroups` workgroups fit the device. */
FAER_HIP_API size_t faer_hip_debug_llt_plan(size_t n, size_t tail_rows, size_t nb2, size_t *starts, size_t cap);
/* ... and what each look-ahead step of that driver is, for the thresholds given (smallest n on the blocked path, rows left to the
 * tail, rows below a panel from which it is solved on the side stream / from which the next diagonal block is updated on the panel
 * stream; the look-ahead streams are assumed to exist).  Four codes per step k in codes[4 k ..]: how P_k gets solved (0 on the side
 * stream by step k - 1, 1 top rows by the follower, 2 on the bulk stream), the trailing update (0 last, 1 merged, 2 band + merged,
 * 3 block column then square beside the side-stream solve), where D_{k+1} is updated (0 nowhere: last, 1 on the bulk stream with
 * the follower's rows, 2 on the panel stream, 3 first on the bulk stream), whether D_{k+1} is factored with a follower (0 / 1).
 * Writes at most `cap` steps and returns their number. */
FAER_HIP_API size_t faer_hip_debug_llt_steps(size_t n, size_t la_min, size_t tail_rows, size_t side_rmin, size_t dpanel_rmin, int *codes,
					     size_t cap);
/* tests: the calling thread's last lblt_factor_in_place -- out = {blocked panels, rows handled by the leaf, 2 x 2 pivots, host
 * synchronisations made inside panels (0 for Partial / PartialDiag; one per rook iteration for Rook / RookDiag)}.
 * For the Full strategy: out[0] = pivot steps run by the multi-workgroup path, out[1] = rows finished by the leaf,
 * out[2] = number of 2 x 2 pivots, out[3] = host synchronisations before the leaf (at most one per 64 launched steps). */
FAER_HIP_API void faer_hip_debug_lblt_last(size_t out[4]);
/* tests: the calling thread's last piv_llt_factor_in_place -- out = {blocked panels, rows handled by the leaf (0: the factorization
 * ended in a panel), columns of L factored (the rank), host synchronisations made inside panels (0)} */
FAER_HIP_API void faer_hip_debug_piv_llt_last(size_t out[4]);
FAER_HIP_API int faer_hip_debug_lu_leaf_width(size_t nrows, FaerHipDType dtype, int resident_workgroups);
/* tests: run every leaf of the partial-pivot LU on the non-cooperative path (the fallback for panels taller than the
 * cooperative kernel can keep resident and for the rerun after an exchange timeout) */
FAER_HIP_API void faer_hip_debug_lu_force_general(int on);
/* tests: switch-over points of the look-ahead LU driver, in rows below the panel (0 = the tuned default): 256-column staged steps
 * below `nb2_from`, pipelined bulk-bound steps from `pipe_from` on, look-ahead at all from `la_min_cols` columns.  Lets a test drive
 * every phase of the driver and the transitions between them at N = 2-6 k; pivots and factors do not depend on the plan. */
FAER_HIP_API void faer_hip_debug_lu_plan(size_t nb2_from, size_t pipe_from, size_t la_min_cols);
/* tests: how many columns the one-pass tall-skinny QR path (csrc/tsqr.hip) completed in the calling thread's last
 * qr_factor_in_place (== ncols: the whole factorization; fewer: a panel was rejected and the classic path finished; -1: the
 * path was not applicable) */
FAER_HIP_API long faer_hip_debug_qr_one_pass_columns(void);
/* tests: which GEMM / TRSM routes the calling thread's library calls took.  One counter per route, thread-local, incremented
 * once per launch decision of gemm_dev / the triangular solves (recursive calls count too; a product can count several routes:
 * the transposed orientation, split-K and a fused epilogue next to its kernel's tile).  faer_hip_debug_route_counts copies at
 * most `cap` counters in enum order and returns FaerHipRoute_Count.  Values are stable: the slots of the in-place tiles, which
 * no driver used and which were removed with their kernels, stay reserved. */
typedef enum FaerHipRoute {
	FaerHipRoute_GemmZeroK = 0,		/* K == 0: fill (Replace) or nothing (Add) */
	FaerHipRoute_GemmRank1 = 1,		/* K == 1 stream */
	FaerHipRoute_GemmGemv = 2,		/* N == 1 or M == 1 stream */
	FaerHipRoute_GemmSkinny = 3,		/* one huge dimension, two tiny ones */
	FaerHipRoute_GemmTransposed = 4,	/* Upper dst, or a row-major Full dst: the product runs on dst^T */
	FaerHipRoute_GemmExtra64 = 5,		/* 64 x 64 kernel for structured operands, diag scaling, index scatter */
	FaerHipRoute_GemmPipe64 = 6,		/* pipelined 64 x 64 tile */
	FaerHipRoute_GemmPipe128 = 7,		/* pipelined 128 x 128 tile */
	FaerHipRoute_GemmPipeWide = 8,		/* pipelined 128 x 256 tile (eight wavefronts) */
	FaerHipRoute_Retired9 = 9,		/* retired (was the in-place product's 32 x 128 tile): reserved, always 0 */
	FaerHipRoute_Retired10 = 10,		/* retired (was the in-place product's 128 x 32 tile): reserved, always 0 */
	FaerHipRoute_GemmLegacy64 = 11,		/* non-pipelined 64 x 64 tile */
	FaerHipRoute_GemmLegacy128 = 12,	/* non-pipelined 128 x 128 tile */
	FaerHipRoute_GemmTriSkipSplit = 13,	/* tri_skip on operands the pipelined loaders cannot address: two plain products */
	FaerHipRoute_GemmSplitK = 14,		/* K split over workgroups + the deterministic reduce */
	FaerHipRoute_GemmTriEnum = 15,		/* square lower dst: only the tiles of the lower triangle are launched */
	FaerHipRoute_GemmFastIo1 = 16,		/* fused epilogue: Replace */
	FaerHipRoute_GemmFastIo2 = 17,		/* fused epilogue: Add, alpha == 1 */
	FaerHipRoute_GemmFastIo3 = 18,		/* fused epilogue: Add, alpha == -1 */
	FaerHipRoute_TrsmTiny = 19,		/* one-wavefront solve (n <= 64, k < 64) */
	FaerHipRoute_TrsmLeafDirect16 = 20,	/* 128-row leaf packing its own triangle, 16 right-hand sides per wavefront */
	FaerHipRoute_TrsmLeafDirect32 = 21,	/* same, 32 right-hand sides per wavefront */
	FaerHipRoute_TrsmLeafPacked16 = 22,	/* 128-row leaf from a packed image (Cholesky), 16 per wavefront */
	FaerHipRoute_TrsmLeafPacked32 = 23,	/* same, 32 per wavefront */
	FaerHipRoute_TrsmRecursion = 24,	/* recursion node: two half solves and one GEMM */
	FaerHipRoute_Count = 25
} FaerHipRoute;
FAER_HIP_API void faer_hip_debug_route_reset(void);
FAER_HIP_API size_t faer_hip_debug_route_counts(long long *out, size_t cap);
/* tests: 1 (default) = the fp32 one-pass QR path (csrc/tsqr.hip) keeps a raw copy of the panel for the launches that read it after V has
 * overwritten it, where the copy fits in 1 GiB; 0 = never (what matrices of more than 4.19 M rows run: V = P M as a launch of its own). */
FAER_HIP_API void faer_hip_debug_qr_panel_copy(int on);
/* tests / A-B measurements: 0 = fp64 matrices never take the one-pass tall-skinny QR path (the classic path of rounds 1-6 runs), 1 (default) =
 * they take it under the same shape rule as fp32 (rows >= 1024, rows >= 3 cols, cols <= 512, unit row stride; columns that are not 16-byte aligned run scalar-access variants of the kernels). */
FAER_HIP_API void faer_hip_debug_qr_one_pass_f64(int on);
/* tests / A-B measurements: 0 = the classic QR path (square / wide matrices, rejected panels) factors its panels by the recursion down to
 * the 8-column cooperative leaf as in rounds 1-6, 1 (default) = a panel of up to 64 columns with at least 256 rows (and 4 rows per column) takes the one-pass
 * panel of csrc/tsqr.hip (and the recursion only if that refuses it). */
FAER_HIP_API void faer_hip_debug_qr_panels_one_pass(int on);
/* tests / A-B measurements: the shape rule of the whole-matrix one-pass QR path -- at least `min_rows` rows and `min_rows_per_column` rows per
 * column (0, 0 = the defaults). */
FAER_HIP_API void faer_hip_debug_qr_one_pass_shape_rule(long min_rows, long min_rows_per_column);
/* Full-pivot LU: 1 = the in-place path (two launches per step) instead of the one-launch-per-step path between two scratch copies
 * (default 0; identical factors and permutations, tests/test_gpu_factor.py). */
FAER_HIP_API void faer_hip_debug_fplu_inplace(int on);
/* tests: 1 = the single-workgroup vector kernels of the tridiagonal / bidiagonal / Hessenberg reductions run their memory-resident bodies
 * at every size (default: from 4096 remaining rows down they keep their columns in registers); results must not depend on it. */
FAER_HIP_API void faer_hip_debug_level2_force_memory_bodies(int on);
/* tests: scratch poisoning.  `byte_or_minus_one` in 0 .. 255: from now on every device scratch buffer the library hands to itself (the
 * pool behind every internal workspace and every staged host operand, all threads) is first filled, over the whole pool buffer and not
 * only the requested size, with that byte, stream ordered like the previous user's last write; -1 (the default) switches it off.  Results
 * must not depend on it: a kernel that reads scratch nothing in the same call has written shows as NaNs (0xFF) or as a difference
 * between two fill bytes (tests/test_gpu_scratch_poison.py).  faer_hip_debug_scratch_fill_stats: out = {fills, bytes filled} since the
 * last faer_hip_debug_scratch_fill. */
FAER_HIP_API void faer_hip_debug_scratch_fill(int byte_or_minus_one);
FAER_HIP_API void faer_hip_debug_scratch_fill_stats(size_t out[2]);
/* host logic of the distributed LU: may a step factor its look-ahead panel of `panel_rows` rows on the CU-masked panel stream? */
FAER_HIP_API int faer_hip_debug_dist_two_streams_ok(size_t panel_rows, FaerHipDType dtype, int panel_cus, int all_cus);
/* Instrumented builds (make -C csrc timing): prints and resets the in-kernel phase counters; a no-op otherwise. */
FAER_HIP_API void faer_hip_debug_dump_timing(void);
/* The internal CU-masked streams themselves (1 = bulk, 2 = panel), for microbenchmarks via faer_hip_set_stream. */
FAER_HIP_API void *faer_hip_debug_internal_stream(int which);
/* Measures `iters` back-to-back launches of the dense GEMM kernel on the calling thread's stream with
 * hipEvents and returns the average milliseconds per launch (operands must be device memory).
 * bench.py uses it for the `roofline` object. */
FAER_HIP_API double faer_hip_time_gemm_ms(FaerHipDType dtype, size_t m, size_t n, size_t k, void *dst, ptrdiff_t dst_cs,
                                          const void *lhs, ptrdiff_t lhs_cs, const void *rhs, ptrdiff_t rhs_cs, int iters);
/* Raw fp64/fp32 MFMA issue-rate probe: every wave of a full-chip grid runs `iters` dependent-free
 * v_mfma 16x16x4 instructions from registers; returns achieved TFLOP/s.  The measured ceiling that
 * roofline fractions are quoted against next to the datasheet peak. */
FAER_HIP_API double faer_hip_mfma_peak_tflops(FaerHipDType dtype, int iters);

/* Kernel-class profile of the calling thread's library calls (bench.py's per-workload `roofline` objects): between
 * faer_hip_prof_begin and faer_hip_prof_end every launch of a dominant kernel class is bracketed by two timing events on
 * the stream it runs on.  prof_end synchronises the device and fills out[3 * cls + {0, 1, 2}] = {milliseconds inside the
 * class's launches, launches, units} for cls = 0 big-tile MFMA products (units: flop), 1 LU panel kernel (columns),
 * 2 one-pass QR update (algorithmic bytes), 3 one-pass QR Gram (bytes), 4 one-pass QR panel kernel (launches),
 * 5 Cholesky leaf (columns).  Measurement aid: the events cost a few microseconds per launch, do not time a profiled call. */
#define FAER_HIP_PROF_CLASSES 6
FAER_HIP_API void faer_hip_prof_begin(void);
FAER_HIP_API void faer_hip_prof_end(double *out_3_x_classes);
/* The same, plus one record of 8 doubles per profiled launch (at most `cap` records; returns how many): {class, ms, units,
 * d0, d1, d2, d3 + 65536 * stream, start in ms after the first recorded launch}.  Class 0 (the MFMA products): d = m, n, k of the
 * product and 0 for a Full, 1 + tri_skip for a Lower destination; stream 0 = the caller's, 1 = bulk, 2 = panel, 3 = side.
 * tools/gpu_update_in_situ.py replays every product of a factorization alone on the same stream from these records. */
FAER_HIP_API size_t faer_hip_prof_end_spans(double *out_3_x_classes, double *spans_8_per_launch, size_t cap);
/* Idle-chip hand-off latency between two resident workgroups on different XCDs, microseconds per one-way hop (tagged
 * 8-byte granule, write-through store -> polling load).  The latency-bound kernels of the LU / Cholesky chains scale
 * with it: bench.py prints it so that a line from a slow box of a pool is recognisable.  < 0: the probe timed out. */
FAER_HIP_API double faer_hip_xwg_hop_us(int iters);

/* Partial-pivot LU on a GPU shared with other work.  The cooperative panel kernel exchanges pivots between resident
 * workgroups; the library arranges their residency itself (one workgroup per compute unit of the stream's CU set, taller
 * panels on a non-cooperative kernel), so on a GPU of its own the exchange cannot stall.  If OTHER work holds compute units
 * for longer than the bounded spin (~0.2 s) the call returns PartialPivLuStatus::Unknown and leaves a partially factored
 * matrix -- for matrices above 512 MiB.  Up to that size the library keeps a copy of its own (< 1 % of the call), restores
 * A after a timeout and finishes on the non-cooperative path, so callers of the reference's FFI surface need nothing.
 * For larger matrices a caller that wants the factorization completed even then lends a copy of the input first:
 * `device_copy` = device memory holding the nrows x ncols matrix (elements of `elem_bytes` = 4 or 8 bytes) column major
 * with leading dimension nrows, valid until the calling thread's NEXT partial_piv_lu call returns.  That call consumes
 * the loan at entry whatever its own shape; a loan made for another shape or scalar type is a precondition violation
 * (abort), never a read with the wrong extent.  After a timeout the call restores A from the copy and factors it on the
 * non-cooperative path (identical pivots, slower). */
FAER_HIP_API void faer_hip_partial_piv_lu_lend_copy(const void *device_copy, size_t nrows, size_t ncols, int elem_bytes);

/* ---------------------------------------------------------------------------------------------
 * 4. Multi-GPU: 1-D block-column partition, one process per GPU.
 *    The caller owns the transport: `bcast` is invoked with device buffers and must broadcast
 *    `bytes` bytes from rank `root` to every rank on the calling thread's stream
 *    (torch.distributed.broadcast over RCCL in bench.py; gloo in the CPU tests).
 * --------------------------------------------------------------------------------------------- */
typedef void (*FaerHipBcastFn)(void *user, void *device_buf, size_t bytes, int root);
/* Optional asynchronous pair: `ibcast` starts the broadcast of `bytes` bytes at `device_buf` from `root` (ordered
 * after the work already enqueued on the calling thread's stream), `wait` makes that stream wait for the broadcast
 * started with the same `slot` (0 .. FAER_HIP_COMM_SLOTS - 1; at most one broadcast per slot is in flight: the LU uses
 * slots 0 / 1, the Cholesky ships a panel in up to four row chunks and alternates two panels, slots 0 .. 7).  `wait` may be
 * called MORE THAN ONCE for the same slot between two `ibcast`s of it (the Cholesky waits for a chunk on every internal
 * stream that reads it) and must then order the calling thread's stream behind the same transfer again.  With both NULL
 * the drivers fall back to the blocking `bcast` (same results, no overlap of transfers with compute). */
#define FAER_HIP_COMM_SLOTS 8
typedef void (*FaerHipIbcastFn)(void *user, void *device_buf, size_t bytes, int root, int slot);
typedef void (*FaerHipWaitFn)(void *user, int slot);
typedef struct FaerHipComm {
	int rank; int world_size; FaerHipBcastFn bcast; void *user; FaerHipIbcastFn ibcast; FaerHipWaitFn wait;
} FaerHipComm;

/* Built-in transport: RCCL broadcasts on a dedicated stream, ordered against the calling thread's stream with events
 * (csrc/rccl_transport.hip).  librccl is dlopen-ed on first use.  Rank 0 obtains the 128-byte ncclUniqueId with
 * faer_hip_rccl_unique_id (0 = ok) and the application ships it to the other ranks; every rank then calls
 * faer_hip_rccl_create (collective) and passes faer_hip_rccl_comm(handle) to the faer_hip_dist_* entry points. */
FAER_HIP_API int faer_hip_rccl_unique_id(void *out_128_bytes);
FAER_HIP_API void *faer_hip_rccl_create(const void *unique_id_128_bytes, int rank, int world_size);
FAER_HIP_API FaerHipComm faer_hip_rccl_comm(void *handle);
FAER_HIP_API void faer_hip_rccl_destroy(void *handle);

/* Number of block columns of width `nb` owned by `rank` out of n columns distributed block-cyclically. */
/* Loop-back transport (TEST infrastructure): the ranks of a distributed factorization as threads of ONE process on ONE GPU, data moved by
 * device-to-device copies; same contract as the RCCL transport (its calls only need the calling thread's current stream), so the stream
 * schedule a rank runs over the built-in transport can be exercised with several ranks on a one-GPU box (tests/test_gpu_dist_threads.py).
 * faer_hip_loopback_group_create once, faer_hip_loopback_rank_create on each rank's thread, faer_hip_loopback_comm(rank_handle) -> comm. */
FAER_HIP_API void *faer_hip_loopback_group_create(int world_size);
FAER_HIP_API void *faer_hip_loopback_rank_create(void *group, int rank);
FAER_HIP_API FaerHipComm faer_hip_loopback_comm(void *rank_handle);
FAER_HIP_API void faer_hip_loopback_stats(void *rank_handle, double *out2);
FAER_HIP_API void faer_hip_loopback_rank_destroy(void *rank_handle);
FAER_HIP_API void faer_hip_loopback_group_destroy(void *group);
FAER_HIP_API size_t faer_hip_dist_local_ncols(size_t n, size_t nb, int rank, int world_size);
/* measurement aids (bench.py --gpus N --workload lu|llt): the calling thread's last faer_hip_dist_* factorization --
 * out3 = {device ms of the whole call, device ms of the panel factorizations this rank owned, their number};
 * faer_hip_rccl_stats: out4 = {ranks the communicator reports (ncclCommCount), broadcasts, bytes, device ms inside
 * ncclBroadcast} since the previous call */
FAER_HIP_API void faer_hip_dist_last_stats(double *out3);
FAER_HIP_API void faer_hip_rccl_stats(void *handle, double *out4);
/* Scalars of device scratch the distributed LU needs: all pivots + two broadcast buffers ({pivots, packed panel}). */
FAER_HIP_API size_t faer_hip_dist_panel_ws_scalars(size_t nrows, size_t nb, FaerHipDType dtype);
/* Distributed partial-pivot LU of an m x n matrix whose block columns (width nb) are dealt block-cyclically
 * over comm.world_size ranks; A_local holds this rank's columns (m x local_ncols, device memory, col-major).
 * perm_fwd / perm_bwd (m entries, u64, HOST memory) are filled on every rank.  `panel_ws` is device scratch of
 * faer_hip_dist_panel_ws_scalars(m, nb) scalars.  Per block column: the owner factors its m_k x nb panel with
 * the single-GPU panel code (same pivoting rule, lu/partial_pivoting/factor.rs:19-187), ONE broadcast ships
 * {pivots, panel}, every rank applies the interchanges, the unit-lower solve and the trailing update to its own
 * columns; look-ahead: the owner of the next block column updates and factors it first and its broadcast
 * overlaps the remaining updates (csrc/dist_lu.h). */
FAER_HIP_API FaerPartialPivLuStatus faer_hip_dist_partial_piv_lu_f64(FaerMatMut A_local, size_t n_global, size_t nb, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerHipComm comm, void *panel_ws);
FAER_HIP_API FaerPartialPivLuStatus faer_hip_dist_partial_piv_lu_f32(FaerMatMut A_local, size_t n_global, size_t nb, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd, FaerHipComm comm, void *panel_ws);


/* Distributed Cholesky (lower) of an n x n matrix, same partition and transport (csrc/dist_llt.h): A_local holds
 * this rank's block columns at full height (n x local_ncols, device memory, col-major; only the lower triangle of
 * the global matrix is referenced or written).  Per block column the owner factors the diagonal block and solves
 * the rows below (cholesky/ldlt/factor.rs:407-433), ONE broadcast ships that column panel, every rank applies
 * lower(A11) -= L10 L10^T (:436-446) to the block columns it owns, with the same look-ahead as the LU.
 * `panel_ws`: device scratch of faer_hip_dist_llt_ws_scalars(n, nb) scalars.  The status is identical on all ranks
 * (NonPositivePivot carries the smallest failing global index). */
FAER_HIP_API size_t faer_hip_dist_llt_ws_scalars(size_t n, size_t nb, FaerHipDType dtype);
FAER_HIP_API FaerLltStatus faer_hip_dist_llt_f64(FaerMatMut A_local, size_t n_global, size_t nb, FaerLltRegularization regularization, FaerHipComm comm, void *panel_ws);
FAER_HIP_API FaerLltStatus faer_hip_dist_llt_f32(FaerMatMut A_local, size_t n_global, size_t nb, FaerLltRegularization regularization, FaerHipComm comm, void *panel_ws);

/* ------------------------------------------------------------------------------------------------
 * Reduction to condensed form, first member: tridiagonalization of a self-adjoint
 * matrix, faer::linalg::evd::tridiag::tridiag_in_place (faer/src/linalg/evd/tridiag.rs:274; the FFI of the reference
 * reaches it only inside self_adjoint_evd, so this entry point is an extension with the Rust function's argument
 * meaning).  A: n x n, only the lower triangle is read or written.  On return its diagonal and subdiagonal hold the
 * tridiagonal T with A = Q T Q^H, the essential parts of the Householder reflectors sit below the subdiagonal and
 * `householder` (block_size x (n - 1), block_size >= 1) holds the block Householder factors of
 * A.submatrix(1, 0, n - 1, n - 1) -- what apply_block_householder_sequence_* consumes (tridiag.rs:516-533, :561-585).
 * Level-2, HBM-bound like the reference (csrc/condense.hip, "Tridiagonalization").  Host or device operands. */
FAER_HIP_API void faer_hip_tridiag_in_place_f64(FaerMatMut A, FaerMatMut householder);
FAER_HIP_API void faer_hip_tridiag_in_place_f32(FaerMatMut A, FaerMatMut householder);

/* Second member: bidiagonalization, faer::linalg::svd::bidiag::bidiag_in_place (faer/src/linalg/svd/bidiag.rs:47).  On
 * return the diagonal and superdiagonal of A hold the upper bidiagonal B with A = U B V^H; the left reflectors sit below
 * the diagonal with their block factors in H_left (bl x min(m, n)), the right reflectors right of the superdiagonal with
 * their block factors in H_right (br x (min(m, n) - 1)) -- the layout apply_block_householder_sequence_* consumes
 * (bidiag.rs:216-254, :404-428).  The reference's SVD only calls it with nrows >= ncols; a wide matrix is processed the
 * way the reference processes it (min(m, n) columns, the last row left normalised without a right reflector).
 * Level-2, HBM-bound like the reference (csrc/condense.hip, "Bidiagonalization").  Host or device operands. */
FAER_HIP_API void faer_hip_bidiag_in_place_f64(FaerMatMut A, FaerMatMut H_left, FaerMatMut H_right);
FAER_HIP_API void faer_hip_bidiag_in_place_f32(FaerMatMut A, FaerMatMut H_left, FaerMatMut H_right);

/* Third member: reduction to upper Hessenberg form, faer::linalg::evd::hessenberg::hessenberg_in_place
 * (faer/src/linalg/evd/hessenberg.rs:549).  A: n x n.  On return the part of A on and above the subdiagonal holds H with
 * A = Q H Q^H, the essential parts of the reflectors sit below the subdiagonal, `householder` (block_size x (n - 1)) holds
 * the block Householder factors of A.submatrix(1, 0, n - 1, n - 1) (hessenberg.rs:382-406, :758-783).  The reference picks
 * an unblocked variant below n = 256 and a blocked one above; both compute the same reflectors in different orders of
 * operations and this entry point agrees with either up to rounding (csrc/condense.hip, "Hessenberg reduction").  Level-2,
 * HBM-bound.  Host or device operands. */
FAER_HIP_API void faer_hip_hessenberg_in_place_f64(FaerMatMut A, FaerMatMut householder);
FAER_HIP_API void faer_hip_hessenberg_in_place_f32(FaerMatMut A, FaerMatMut householder);

/* ------------------------------------------------------------------------------------------------
 * Modifying an existing Cholesky factorization (faer/src/linalg/cholesky/llt/update.rs:360 rank_r_update_clobber,
 * cholesky/ldlt/update.rs:376 rank_r_update_clobber and :417 delete_rows_and_cols_clobber; the FFI of the reference does not
 * export them, so these entry points are extensions with the Rust functions' argument meaning).  Real scalars.
 *   rank_r_update_clobber: L (n x n, the factor of A in its lower triangle; for LDLT unit lower L with D on the diagonal), W (n x r),
 *     alpha (r entries).  On return the lower triangle of L holds the factor of A + W diag(alpha) W^T; a negative alpha downdates.
 *     W and alpha are clobbered (contents unspecified).  The LLT returns NonPositivePivot{index} with the reference's index when a
 *     new pivot is not positive (a NaN passes, as in the reference); L, W and alpha are unspecified then.
 *   delete_rows_and_cols_clobber: `indices` (host memory, u32 or u64, sorted in place) names the rows and columns to remove.  On
 *     return the leading (n - r)^2 block of LD holds the factors of A without them; the trailing r rows are unspecified.
 *     `mem` is ignored; the _scratch query returns the reference's figure (dim * n_removed + n_removed scalars).
 * L / LD, W and alpha may each be host or device memory with arbitrary element strides.  Only the lower triangle of a device L is read
 * or written, and no byte outside a view is written.  n == 0, r == 0 and an empty index list return at once without touching the device.
 * The call runs on the caller's stream and takes all its device memory from one arena (csrc/chol_update.hip). */
FAER_HIP_API FaerLltStatus faer_hip_llt_rank_r_update_clobber_f64(FaerMatMut L, FaerMatMut W, FaerVecMut alpha);
FAER_HIP_API FaerLltStatus faer_hip_llt_rank_r_update_clobber_f32(FaerMatMut L, FaerMatMut W, FaerVecMut alpha);
FAER_HIP_API void faer_hip_ldlt_rank_r_update_clobber_f64(FaerMatMut LD, FaerMatMut W, FaerVecMut alpha);
FAER_HIP_API void faer_hip_ldlt_rank_r_update_clobber_f32(FaerMatMut LD, FaerMatMut W, FaerVecMut alpha);
FAER_HIP_API void faer_hip_ldlt_delete_rows_and_cols_clobber_u32_f64(FaerMatMut LD, FaerSliceMut indices, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void faer_hip_ldlt_delete_rows_and_cols_clobber_u64_f64(FaerMatMut LD, FaerSliceMut indices, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void faer_hip_ldlt_delete_rows_and_cols_clobber_u32_f32(FaerMatMut LD, FaerSliceMut indices, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API void faer_hip_ldlt_delete_rows_and_cols_clobber_u64_f32(FaerMatMut LD, FaerSliceMut indices, FaerPar par, FaerMemAlloc mem);
FAER_HIP_API FaerLayout faer_hip_ldlt_delete_rows_and_cols_clobber_scratch_f64(size_t dim, size_t n_removed);
FAER_HIP_API FaerLayout faer_hip_ldlt_delete_rows_and_cols_clobber_scratch_f32(size_t dim, size_t n_removed);
/* tests: the calling thread's last call of the family -- out = {column blocks, tail launches, chunks of W per block, host
 * synchronisations inside the block loop (0)} */
FAER_HIP_API void faer_hip_debug_chol_update_last(long out[4]);
/* measurement aid (tools/bench_chol_update.py): 1 = only the diagonal kernels of the family run -- the serial chain of a call; the
 * factor it leaves is wrong.  Process wide, 0 by default. */
FAER_HIP_API void faer_hip_debug_chol_update_diag_only(int on);
/* out = {NB: columns per block, RC: columns of W per chunk}; dtype: a FaerHipDType code.  Needs no device. */
FAER_HIP_API void faer_hip_chol_update_shape(int dtype, size_t out[2]);

/* Complex partial-pivot LU (cgetrf.hip).
 * out = {W: columns per panel, the row count of the tallest panel the LDS-resident leaf takes}; dtype: FaerHipDType_C32 / _C64.
 * Needs no device. */
FAER_HIP_API void faer_hip_debug_clu_shape(int dtype, size_t out[2]);
/* tests: the calling thread's last complex partial_piv_lu_factor_in_place -- out = {panels on the LDS leaf, panels on the
 * column-step kernels, column-step launches, interchange launches} */
FAER_HIP_API void faer_hip_debug_clu_last(size_t out[4]);

/* Complex triangular inverse (ctrtri.hip).
 * out = {E: edge of the LDS-resident leaf, the number of sub-blocks along that edge -- the leaf inverts E / out[1]-wide diagonal
 * sub-blocks by substitution and combines them by doubling}; elem_bytes: 8 (c32) or 16 (c64).  Needs no device. */
FAER_HIP_API void faer_hip_debug_ctrtri_shape(int elem_bytes, size_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* FAER_HIP_H */
