// extern "C" surface of libfaer_hip.so (see include/faer_hip.h for the contract and the reference
// citations of every entry point).  This file only validates shapes, stages host operands and forwards
// to the device drivers; there is deliberately no CPU compute path here.
#include <algorithm>
#include <atomic>
#include <limits>

#include "arena.h"
#include "common.h"
#include "perm.h"

using namespace fh;

namespace {

std::atomic<int> g_par_tag{(int) FaerParTag_Rayon};
std::atomic<size_t> g_par_threads{0};

// ---- matmul ---------------------------------------------------------------------------------------
template <typename T> void matmul_api(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha)
{
	// faer/src/linalg/matmul/mod.rs:1562-1575 `precondition`
	FH_CHECK(C.nrows == A.nrows && C.ncols == B.ncols && A.ncols == B.nrows, "matmul: dimension mismatch");
	FH_CHECK(alpha != nullptr, "matmul: alpha is NULL");
	const bool add = accum == FaerAccum_Add;
	Staged<const T> a(view<T>(A), true, false), b(view<T>(B), true, false);
	Staged<T> c(view<T>(C), add, true); // Replace never reads dst
	gemm_dev<T>(c.dev, DST_FULL, add, a.dev, b.dev, *static_cast<const T *>(alpha));
}

template <typename T>
void matmul_triangular_api(FaerMatMut C, FaerBlock cb, FaerAccum accum, FaerMatRef A, FaerBlock ab, FaerMatRef B, FaerBlock bb,
			   const void *alpha)
{
	FH_CHECK(C.nrows == A.nrows && C.ncols == B.ncols && A.ncols == B.nrows, "matmul_triangular: dimension mismatch");
	// triangular operands must be square (faer/src/linalg/matmul/triangular.rs:1246-1262)
	FH_CHECK(cb == FaerBlock_Rectangular || C.nrows == C.ncols, "matmul_triangular: triangular dst must be square");
	FH_CHECK(ab == FaerBlock_Rectangular || A.nrows == A.ncols, "matmul_triangular: triangular lhs must be square");
	FH_CHECK(bb == FaerBlock_Rectangular || B.nrows == B.ncols, "matmul_triangular: triangular rhs must be square");
	const bool add = accum == FaerAccum_Add;
	Staged<const T> a(view<T>(A), true, false), b(view<T>(B), true, false);
	// a triangular dst keeps its other triangle => always copy in
	Staged<T> c(view<T>(C), add || cb != FaerBlock_Rectangular, true);
	matmul_triangular_dev<T>(c.dev, (int) cb, add, a.dev, (int) ab, b.dev, (int) bb, *static_cast<const T *>(alpha));
}

// conj: complex scalars only (conjugation is the identity for real ones)
template <typename T> void trsm_api(FaerMatRef Tm, FaerMatMut rhs, bool upper, bool unit, bool conj = false)
{
	FH_CHECK(Tm.nrows == Tm.ncols && rhs.nrows == Tm.ncols, "triangular solve: dimension mismatch");
	Staged<const T> t(view<T>(Tm), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	if constexpr (is_cx<T>::value)
		ctrsm_dev(t.dev, upper, unit, conj, x.dev);
	else if (upper)
		trsm_upper_dev<T>(t.dev, unit, x.dev);
	else
		trsm_lower_dev<T>(t.dev, unit, x.dev);
}

template <typename T> FaerLltStatus llt_api(FaerMatMut A, FaerLltRegularization reg)
{
	FH_CHECK(A.nrows == A.ncols, "llt: matrix must be square");
	T delta = reg.dynamic_regularization_delta ? *static_cast<const T *>(reg.dynamic_regularization_delta) : (T) 0;
	T eps = reg.dynamic_regularization_epsilon ? *static_cast<const T *>(reg.dynamic_regularization_epsilon) : (T) 0;
	long r;
	{
		Staged<T> a(view<T>(A), true, true);
		r = potrf_lower_dev<T>(a.dev, delta, eps);
	}
	FaerLltStatus st;
	memset(&st, 0, sizeof(st));
	if (r >= 0) {
		st.tag = FaerLltStatus_Ok;
		st.ok.dynamic_regularization_count = (size_t) r;
	} else {
		st.tag = FaerLltStatus_NonPositivePivot;
		st.non_positive_pivot.index = (size_t) (-r - 1);
	}
	return st;
}

template <typename T> FaerLdltStatus ldlt_api(FaerMatMut A, FaerLdltRegularization reg)
{
	FH_CHECK(A.nrows == A.ncols, "ldlt: matrix must be square");
	T delta = reg.dynamic_regularization_delta ? *static_cast<const T *>(reg.dynamic_regularization_delta) : (T) 0;
	T eps = reg.dynamic_regularization_epsilon ? *static_cast<const T *>(reg.dynamic_regularization_epsilon) : (T) 0;
	const signed char *signs = static_cast<const signed char *>(reg.dynamic_regularization_signs.ptr);
	if (signs) {
		FH_CHECK(reg.dynamic_regularization_signs.len >= A.nrows, "ldlt: the sign slice is shorter than the matrix");
		FH_CHECK(!is_device_ptr(signs), "ldlt: the sign slice must be host memory");
	}
	long r;
	{
		Staged<T> a(view<T>(A), true, true);
		r = sytrf_lower_dev<T>(a.dev, delta, eps, signs);
	}
	FaerLdltStatus st;
	memset(&st, 0, sizeof(st));
	if (r >= 0) {
		st.tag = FaerLdltStatus_Ok;
		st.ok.dynamic_regularization_count = (size_t) r;
	} else {
		st.tag = FaerLdltStatus_ZeroPivot;
		st.zero_pivot.index = (size_t) (-r - 1);
	}
	return st;
}

// cholesky/ldlt/solve.rs:12-50: L y = b (unit lower), y <- D^-1 y, L^H x = y
template <typename T> void ldlt_solve_api(FaerMatRef L, FaerVecRef D, FaerMatMut rhs)
{
	FH_CHECK(L.nrows == L.ncols && rhs.nrows == L.nrows && D.len == L.nrows, "ldlt solve: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<const T> d(vview<T>(D), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	trsm_lower_dev<T>(l.dev, true, x.dev);
	scale_rows_recip_dev<T>(x.dev, d.dev.p, d.dev.rs);
	trsm_upper_dev<T>(l.dev.t(), true, x.dev);
}

template <typename T> void llt_solve_api(FaerMatRef L, FaerMatMut rhs)
{
	// cholesky/llt/solve.rs:12-35: L y = b ; L^H x = y
	FH_CHECK(L.nrows == L.ncols && rhs.nrows == L.nrows, "llt solve: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	trsm_lower_dev<T>(l.dev, false, x.dev);
	trsm_upper_dev<T>(l.dev.t(), false, x.dev);
}

template <typename T, typename I> FaerPartialPivLuStatus lu_api(FaerMatMut A, FaerSliceMut pf, FaerSliceMut pb)
{
	const idx_t m = (idx_t) A.nrows;
	std::vector<idx_t> perm((size_t) m), perm_inv((size_t) m);
	long nt;
	{
		Staged<T> a(view<T>(A), true, true);
		nt = getrf_dev<T>(a.dev, perm.data(), perm_inv.data());
		if (nt < 0)
			a.writeback = false; // Unknown (exchange timeout without room for the rerun): a host operand keeps its input
	}
	store_perm<I>("partial_piv_lu", pf, pb, perm.data(), perm_inv.data(), m);
	FaerPartialPivLuStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = nt >= 0 ? FaerPartialPivLuStatus_Ok : FaerPartialPivLuStatus_Unknown; // Unknown: exchange timeout (getrf.hip)
	st.ok.transposition_count = nt >= 0 ? (size_t) nt : 0;
	return st;
}

size_t qr_block_size(size_t nrows, size_t ncols)
{
	// qr/no_pivoting/factor.rs:91-116
	const size_t prod = nrows * ncols;
	const size_t size = nrows < ncols ? nrows : ncols;
	size_t r;
	if (prod > 8192UL * 8192)
		r = 256;
	else if (prod > 2048UL * 2048)
		r = 128;
	else if (prod > 1024UL * 1024)
		r = 64;
	else if (prod > 512UL * 512)
		r = 48;
	else if (prod > 128UL * 128)
		r = 32;
	else if (prod > 32UL * 32)
		r = 8;
	else if (prod > 16UL * 16)
		r = 4;
	else
		r = 1;
	if (r > size)
		r = size;
	return r < 1 ? 1 : r;
}

template <typename T> FaerQrStatus qr_api(FaerMatMut A, FaerMatMut Q, FaerQrParams params)
{
	const size_t size = A.nrows < A.ncols ? A.nrows : A.ncols;
	FH_CHECK(Q.nrows > 0 && Q.ncols == size, "qr: Q_coeff must be block_size x min(nrows, ncols)");
	long rank;
	{
		Staged<T> a(view<T>(A), true, true);
		// (copied in: the factorization writes the upper triangles of Q_coeff's diagonal blocks only, the rest keeps the caller's values
		// as it does for a device operand -- staged without copy-in, stale scratch bytes went back to the host in those cells)
		Staged<T> q(view<T>(Q), true, true);
		rank = geqrf_dev<T>(a.dev, q.dev, (idx_t) params.blocking_threshold);
	}
	FaerQrStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerQrStatus_Ok;
	st.ok.rank = (size_t) rank;
	return st;
}

template <typename T> void apply_hh_api(FaerMatRef V, FaerMatRef H, FaerMatMut rhs, bool transpose)
{
	const size_t size = V.nrows < V.ncols ? V.nrows : V.ncols;
	FH_CHECK(H.nrows > 0 && H.ncols == size && rhs.nrows == V.nrows, "apply_householder: dimension mismatch");
	Staged<const T> v(view<T>(V), true, false), h(view<T>(H), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	apply_householder_sequence_left_dev<T>(v.dev, h.dev, x.dev, transpose);
}

// lu/partial_pivoting/solve.rs:20-50 and :52-80; conj (complex scalars only): the system is conj(A) X = B / conj(A)^T X = B
template <typename T, typename I>
void lu_solve_api(FaerMatRef L, FaerMatRef U, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs, bool transpose, bool conj = false)
{
	const size_t n = L.nrows;
	FH_CHECK(L.ncols == n && U.nrows == n && U.ncols == n && rhs.nrows == n, "partial_piv_lu solve: dimension mismatch");
	check_perm_slice("partial_piv_lu solve", transpose ? pf : pb, (idx_t) n); // (the one that is not used)
	DevPerm perm("partial_piv_lu solve", transpose ? pb : pf, (idx_t) n, I{});
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	if constexpr (is_cx<T>::value) {
		if (!transpose) {
			permute_rows<T>(x.dev, perm);
			ctrsm_dev(l.dev, false, true, conj, x.dev);
			ctrsm_dev(u.dev, true, false, conj, x.dev);
		} else {
			ctrsm_dev(u.dev.t(), false, false, conj, x.dev);
			ctrsm_dev(l.dev.t(), true, true, conj, x.dev);
			permute_rows<T>(x.dev, perm); // the inverse permutation
		}
	} else if (!transpose) {
		permute_rows<T>(x.dev, perm);
		trsm_lower_dev<T>(l.dev, true, x.dev);
		trsm_upper_dev<T>(u.dev, false, x.dev);
	} else {
		trsm_lower_dev<T>(u.dev.t(), false, x.dev);
		trsm_upper_dev<T>(l.dev.t(), true, x.dev);
		permute_rows<T>(x.dev, perm); // the inverse permutation
	}
}

// the three read-only operands of the QR solver side, staged once
template <typename T> struct QrFactors {
	Staged<const T> qb, qc, r;
	QrFactors(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R) : qb(view<T>(Qb), true, false), qc(view<T>(Qc), true, false), r(view<T>(R), true, false) {}
};

// qr/no_pivoting/solve.rs:38-75 (lstsq / square) and :140-175 (transpose)
void qr_solve_check(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerMatMut rhs, bool transpose, bool square)
{
	const size_t m = Qb.nrows, n = Qb.ncols;
	const size_t size = m < n ? m : n;
	FH_CHECK(Qc.nrows > 0 && rhs.nrows == m && m >= n && Qc.ncols == size && R.nrows >= size && R.ncols == n,
		 "qr solve: dimension mismatch");
	if (square || transpose)
		FH_CHECK(m == n && R.nrows == n, "qr solve: the factorization must be square");
}
template <typename T> void qr_solve_dev(MatV<const T> Qb, MatV<const T> Qc, MatV<const T> R, MatV<T> X, bool transpose)
{
	const idx_t n = Qb.ncols; // (== min(nrows, ncols): qr_solve_check)
	MatV<const T> Rtop = R.sub(0, 0, n, n);
	if (!transpose) {
		apply_householder_sequence_left_dev<T>(Qb, Qc, X, true); // Q^H rhs
		trsm_upper_dev<T>(Rtop, false, X.sub(0, 0, n, X.ncols));
	} else {
		trsm_lower_dev<T>(Rtop.t(), false, X);
		apply_householder_sequence_left_dev<T>(Qb, Qc, X, false); // Q rhs
	}
}
template <typename T> void qr_solve_api(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerMatMut rhs, bool transpose, bool square)
{
	qr_solve_check(Qb, Qc, R, rhs, transpose, square);
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> x(view<T>(rhs), true, true);
	qr_solve_dev<T>(f.qb.dev, f.qc.dev, f.r.dev, x.dev, transpose);
}

// ---- triangular inverse (triangular_inverse.rs:43-230): dst's other triangle (and, unit: its diagonal) is untouched
template <typename T> void tri_inverse_api(FaerMatMut Out, FaerMatRef Tm, bool upper, bool unit)
{
	FH_CHECK(Tm.nrows == Tm.ncols && Out.nrows == Tm.nrows && Out.ncols == Tm.ncols, "triangular inverse: dimension mismatch");
	Staged<const T> t(view<T>(Tm), true, false);
	Staged<T> o(view<T>(Out), true, true); // keeps the triangle that is not written
	if (upper)
		tri_invert_lower_dev<T>(o.dev.t(), t.dev.t(), unit);
	else
		tri_invert_lower_dev<T>(o.dev, t.dev, unit);
}

// cholesky/llt/reconstruct.rs:14-40: lower(out) = L L^H
template <typename T> void llt_reconstruct_api(FaerMatMut Out, FaerMatRef L)
{
	FH_CHECK(L.nrows == L.ncols && Out.nrows == L.nrows && Out.ncols == L.nrows, "llt reconstruct: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<T> o(view<T>(Out), true, true);
	matmul_triangular_dev<T>(o.dev, 1, false, l.dev, 1, l.dev.t(), 2, (T) 1);
}

// cholesky/llt/inverse.rs:14-47: lower(out) = W^H W, W = inv(L)
template <typename T> void llt_inverse_api(FaerMatMut Out, FaerMatRef L)
{
	const idx_t n = (idx_t) L.nrows;
	FH_CHECK(L.nrows == L.ncols && Out.nrows == L.nrows && Out.ncols == L.nrows, "llt inverse: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<T> o(view<T>(Out), true, true);
	Scratch wb((size_t) n * (size_t) n * sizeof(T) + 256);
	MatV<T> W{wb.as<T>(), n, n, 1, n};
	tri_invert_lower_dev<T>(W, l.dev, false);
	matmul_triangular_dev<T>(o.dev, 1, false, W.t().c(), 2, W.c(), 1, (T) 1);
	ctx().sync();
}

// cholesky/ldlt/reconstruct.rs:14-62: lower(out) = (L D) L^H, L unit lower
template <typename T> void ldlt_reconstruct_api(FaerMatMut Out, FaerMatRef L, FaerVecRef D)
{
	const idx_t n = (idx_t) L.nrows;
	FH_CHECK(L.nrows == L.ncols && Out.nrows == L.nrows && Out.ncols == L.nrows && D.len == L.nrows, "ldlt reconstruct: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<const T> d(vview<T>(D), true, false);
	Staged<T> o(view<T>(Out), true, true);
	Scratch wb((size_t) n * (size_t) n * sizeof(T) + 256);
	MatV<T> LxD{wb.as<T>(), n, n, 1, n};
	ldlt_scale_lower_dev<T>(LxD, l.dev, d.dev.p, d.dev.rs);
	matmul_triangular_dev<T>(o.dev, 1, false, LxD.c(), 1, l.dev.t(), 6, (T) 1);
	ctx().sync();
}

// cholesky/ldlt/inverse.rs:14-62: lower(out) = (W^H D^-1) W, W = inv(L) unit lower
template <typename T> void ldlt_inverse_api(FaerMatMut Out, FaerMatRef L, FaerVecRef D)
{
	const idx_t n = (idx_t) L.nrows;
	FH_CHECK(L.nrows == L.ncols && Out.nrows == L.nrows && Out.ncols == L.nrows && D.len == L.nrows, "ldlt inverse: dimension mismatch");
	Staged<const T> l(view<T>(L), true, false);
	Staged<const T> d(vview<T>(D), true, false);
	Staged<T> o(view<T>(Out), true, true);
	Scratch wb((size_t) n * (size_t) n * sizeof(T) + 256);
	MatV<T> W{wb.as<T>(), n, n, 1, n};
	tri_invert_lower_dev<T>(W, l.dev, true);
	ldlt_inverse_prepare_dev<T>(W, d.dev.p, d.dev.rs);
	matmul_triangular_dev<T>(o.dev, 1, false, W.c(), 2, W.c(), 5, (T) 1);
	ctx().sync();
}

// lu/partial_pivoting/reconstruct.rs:17-83: out = P^-1 (L U)
template <typename T, typename I> void lu_reconstruct_api(FaerMatMut Out, FaerMatRef L, FaerMatRef U, FaerSliceRef pf, FaerSliceRef pb)
{
	const idx_t m = (idx_t) L.nrows, n = (idx_t) U.ncols;
	const idx_t size = m < n ? m : n;
	FH_CHECK(Out.nrows == L.nrows && Out.ncols == U.ncols && (idx_t) L.ncols >= size && (idx_t) U.nrows >= size,
		 "partial_piv_lu reconstruct: dimension mismatch");
	check_perm_slice("partial_piv_lu reconstruct", pf, m);
	DevPerm perm_bwd("partial_piv_lu reconstruct", pb, m, I{});
	if (m == 0 || n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> o(view<T>(Out), false, true);
	Scratch tb((size_t) m * (size_t) n * sizeof(T));
	MatV<T> tmp{tb.as<T>(), m, n, 1, m};
	matmul_triangular_dev<T>(tmp.sub(0, 0, size, size), 0, false, l.dev.sub(0, 0, size, size), 5, u.dev.sub(0, 0, size, size), 2, (T) 1);
	if (m > n)
		matmul_triangular_dev<T>(tmp.sub(size, 0, m - size, size), 0, false, l.dev.sub(size, 0, m - size, size), 0, u.dev.sub(0, 0, size, size), 2,
					 (T) 1);
	if (m < n)
		matmul_triangular_dev<T>(tmp.sub(0, size, size, n - size), 0, false, l.dev.sub(0, 0, size, size), 5, u.dev.sub(0, size, size, n - size), 0,
					 (T) 1);
	gather_rows_dev<T>(o.dev, tmp.c(), perm_bwd.dev()); // permute_rows(out, tmp, perm.inverse()): out[i, :] = tmp[perm_bwd[i], :]
	ctx().sync();
}

// lu/partial_pivoting/inverse.rs:15-62: out = U^-1 L^-1 P
template <typename T, typename I> void lu_inverse_api(FaerMatMut Out, FaerMatRef L, FaerMatRef U, FaerSliceRef pf, FaerSliceRef pb)
{
	const idx_t n = (idx_t) L.ncols;
	FH_CHECK((idx_t) L.nrows == n && (idx_t) U.nrows == n && (idx_t) U.ncols == n && (idx_t) Out.nrows == n && (idx_t) Out.ncols == n,
		 "partial_piv_lu inverse: dimension mismatch");
	check_perm_slice("partial_piv_lu inverse", pf, n);
	DevPerm perm_bwd("partial_piv_lu inverse", pb, n, I{});
	if (n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> o(view<T>(Out), false, true);
	Scratch tb((size_t) n * (size_t) n * sizeof(T));
	MatV<T> tmp{tb.as<T>(), n, n, 1, n};
	tri_invert_lower_dev<T>(o.dev, l.dev, true);	  // strict lower part of out
	tri_invert_lower_dev<T>(o.dev.t(), u.dev.t(), false); // upper part (with diagonal) of out
	matmul_triangular_dev<T>(tmp, 0, false, o.dev.c(), 2, o.dev.c(), 5, (T) 1);
	gather_rows_dev<T>(o.dev.t(), tmp.t().c(), perm_bwd.dev()); // permute_cols(out, tmp, perm.inverse()): out[:, j] = tmp[:, perm_bwd[j]]
	ctx().sync();
}

// qr/no_pivoting/reconstruct.rs:18-52: out = Q [R; 0]
void qr_reconstruct_check(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R)
{
	const idx_t m = (idx_t) Qb.nrows, n = (idx_t) R.ncols;
	const idx_t size = m < n ? m : n;
	FH_CHECK((idx_t) Out.nrows == m && (idx_t) Out.ncols == n && (idx_t) Qb.ncols == size && (idx_t) Qc.ncols == size && (idx_t) R.nrows == size &&
			 Qc.nrows > 0,
		 "qr reconstruct: dimension mismatch");
}
template <typename T> void qr_reconstruct_dev(MatV<T> Out, MatV<const T> Qb, MatV<const T> Qc, MatV<const T> R)
{
	zero_then_upper_dev<T>(Out, &R);
	apply_householder_sequence_left_dev<T>(Qb, Qc, Out, false);
}
template <typename T> void qr_reconstruct_api(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R)
{
	qr_reconstruct_check(Out, Qb, Qc, R);
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> o(view<T>(Out), false, true);
	qr_reconstruct_dev<T>(o.dev, f.qb.dev, f.qc.dev, f.r.dev);
}

// qr/no_pivoting/inverse.rs:17-58: out = R^-1 Q^H
void qr_inverse_check(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R)
{
	const idx_t n = (idx_t) Qb.ncols;
	FH_CHECK(Qc.nrows > 0 && (idx_t) Qb.nrows == n && (idx_t) Qc.ncols == n && (idx_t) R.nrows == n && (idx_t) R.ncols == n &&
			 (idx_t) Out.nrows == n && (idx_t) Out.ncols == n,
		 "qr inverse: dimension mismatch");
}
template <typename T> void qr_inverse_dev(MatV<T> Out, MatV<const T> Qb, MatV<const T> Qc, MatV<const T> R)
{
	zero_then_upper_dev<T>(Out, nullptr);
	tri_invert_lower_dev<T>(Out.t(), R.t(), false);
	// out <- out Q^H  ==  (Q out^T)^T   (householder.rs:836-854)
	apply_householder_sequence_left_dev<T>(Qb, Qc, Out.t(), false);
}
template <typename T> void qr_inverse_api(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R)
{
	qr_inverse_check(Out, Qb, Qc, R);
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> o(view<T>(Out), false, true);
	qr_inverse_dev<T>(o.dev, f.qb.dev, f.qc.dev, f.r.dev);
}

// householder.rs:813-854: M <- M Q (transpose == false) or M Q^H (transpose == true), as left applications on M^T
template <typename T> void apply_hh_right_api(FaerMatRef V, FaerMatRef H, FaerMatMut M, bool transpose)
{
	const size_t size = V.nrows < V.ncols ? V.nrows : V.ncols;
	FH_CHECK(H.nrows > 0 && H.ncols == size && M.ncols == V.nrows, "apply_householder (right): dimension mismatch");
	Staged<const T> v(view<T>(V), true, false), h(view<T>(H), true, false);
	Staged<T> x(view<T>(M), true, true);
	apply_householder_sequence_left_dev<T>(v.dev, h.dev, x.dev.t(), !transpose);
}

// lu/full_pivoting/factor.rs:452-525
template <typename T, typename I>
FaerFullPivLuStatus full_lu_api(FaerMatMut A, FaerSliceMut rpf, FaerSliceMut rpb, FaerSliceMut cpf, FaerSliceMut cpb)
{
	const idx_t m = (idx_t) A.nrows, n = (idx_t) A.ncols;
	std::vector<idx_t> rp((size_t) m), rpi((size_t) m), cp((size_t) n), cpi((size_t) n);
	long nt;
	{
		Staged<T> a(view<T>(A), true, true);
		nt = full_piv_lu_dev<T>(a.dev, rp.data(), rpi.data(), cp.data(), cpi.data());
	}
	store_perm<I>("full_piv_lu", rpf, rpb, rp.data(), rpi.data(), m);
	store_perm<I>("full_piv_lu", cpf, cpb, cp.data(), cpi.data(), n);
	FaerFullPivLuStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerFullPivLuStatus_Ok;
	st.ok.transposition_count = (size_t) nt;
	return st;
}

// lu/full_pivoting/solve.rs: A x = b (:22-60) and A^T x = b (:75-110)
template <typename T, typename I>
void full_lu_solve_api(FaerMatRef L, FaerMatRef U, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf, FaerSliceRef cpb, FaerMatMut rhs,
		       bool transpose)
{
	const size_t n = L.nrows;
	const char *who = "full_piv_lu solve";
	FH_CHECK(L.ncols == n && U.nrows == n && U.ncols == n && rhs.nrows == n, "full_piv_lu solve: dimension mismatch");
	check_perm_slice(who, transpose ? rpf : rpb, (idx_t) n); // (the two that are not used)
	check_perm_slice(who, transpose ? cpb : cpf, (idx_t) n);
	// A x = b: row_perm, then col_perm.inverse(); A^T x = b: col_perm, then row_perm.inverse()
	DevPerm first(who, transpose ? cpf : rpf, (idx_t) n, I{}), last(who, transpose ? rpb : cpb, (idx_t) n, I{});
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	permute_rows<T>(x.dev, first);
	if (!transpose) {
		trsm_lower_dev<T>(l.dev, true, x.dev);
		trsm_upper_dev<T>(u.dev, false, x.dev);
	} else {
		trsm_lower_dev<T>(u.dev.t(), false, x.dev);
		trsm_upper_dev<T>(l.dev.t(), true, x.dev);
	}
	permute_rows<T>(x.dev, last);
}

// evd/tridiag.rs:274-299
template <typename T> void tridiag_api(FaerMatMut A, FaerMatMut Hh)
{
	FH_CHECK(A.nrows == A.ncols, "tridiag: the matrix must be square");
	FH_CHECK(Hh.ncols == (A.nrows > 0 ? A.nrows - 1 : 0), "tridiag: householder must have n - 1 columns"); // tridiag.rs:287
	if (A.nrows == 0)
		return; // :288-290
	FH_CHECK(Hh.nrows > 0 || A.nrows == 1, "tridiag: householder must have at least one row");
	if (A.nrows == 1)
		return;
	Staged<T> a(view<T>(A), true, true);
	Staged<T> h(view<T>(Hh), true, true); // only the block upper triangles are written
	tridiag_dev<T>(a.dev, h.dev);
}

// evd/hessenberg.rs:549-566
template <typename T> void hessenberg_api(FaerMatMut A, FaerMatMut Hh)
{
	FH_CHECK(A.nrows == A.ncols, "hessenberg: the matrix must be square");
	FH_CHECK(Hh.ncols == (A.nrows > 0 ? A.nrows - 1 : 0), "hessenberg: householder must have n - 1 columns"); // :557-560
	if (A.nrows <= 1)
		return;
	Staged<T> a(view<T>(A), true, true);
	Staged<T> h(view<T>(Hh), true, true); // only the block upper triangles are written
	hessenberg_dev<T>(a.dev, h.dev);
}

// svd/bidiag.rs:47-66
template <typename T> void bidiag_api(FaerMatMut A, FaerMatMut Hl, FaerMatMut Hr)
{
	const size_t size = A.nrows < A.ncols ? A.nrows : A.ncols;
	FH_CHECK(Hl.ncols == size && Hr.ncols == (size > 0 ? size - 1 : 0), "bidiag: H_left / H_right must have min(m, n) and min(m, n) - 1 columns"); // :60-61
	if (size == 0)
		return;
	Staged<T> a(view<T>(A), true, true);
	Staged<T> hl(view<T>(Hl), true, true), hr(view<T>(Hr), true, true); // only the block upper triangles are written
	bidiag_dev<T>(a.dev, hl.dev, hr.dev);
}

// qr/col_pivoting/factor.rs:356-395
template <typename T, typename I> FaerColPivQrStatus colpiv_qr_api(FaerMatMut A, FaerMatMut Q, FaerSliceMut pf, FaerSliceMut pb)
{
	const idx_t n = (idx_t) A.ncols;
	const size_t size = A.nrows < A.ncols ? A.nrows : A.ncols;
	FH_CHECK(Q.nrows > 0 && Q.ncols == size, "colpiv_qr: Q_coeff must be block_size x min(nrows, ncols)");
	std::vector<idx_t> cp((size_t) n), cpi((size_t) n);
	long nt;
	{
		Staged<T> a(view<T>(A), true, true);
		// (copied in: the factorization writes the upper triangles of Q_coeff's diagonal blocks only, the rest keeps the caller's values
		// as it does for a device operand -- staged without copy-in, stale scratch bytes went back to the host in those cells)
		Staged<T> q(view<T>(Q), true, true);
		nt = colpiv_qr_dev<T>(a.dev, q.dev, cp.data(), cpi.data());
	}
	store_perm<I>("colpiv_qr", pf, pb, cp.data(), cpi.data(), n);
	FaerColPivQrStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerColPivQrStatus_Ok;
	st.ok.transposition_count = (size_t) nt;
	return st;
}

// qr/col_pivoting/solve.rs:52-80 (lstsq / square) and :158-184 (transpose)
template <typename T, typename I>
void colpiv_qr_solve_api(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs, bool transpose, bool square)
{
	const idx_t n = (idx_t) Qb.ncols;
	check_perm_slice("colpiv_qr solve", transpose ? pb : pf, n); // (the one that is not used)
	qr_solve_check(Qb, Qc, R, rhs, transpose, square);
	DevPerm perm("colpiv_qr solve", transpose ? pf : pb, n, I{});
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> x(view<T>(rhs), true, true);
	if (transpose)
		permute_rows<T>(x.dev, perm);
	qr_solve_dev<T>(f.qb.dev, f.qc.dev, f.r.dev, x.dev, transpose);
	if (!transpose)
		permute_rows<T>(x.dev.sub(0, 0, n, x.dev.ncols), perm); // col_perm.inverse() on the rows of the solution
}

// lu/full_pivoting/reconstruct.rs: out(i, j) = (L U)(row_perm_inv[i], col_perm_inv[j])
template <typename T, typename I>
void full_lu_reconstruct_api(FaerMatMut Out, FaerMatRef L, FaerMatRef U, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf, FaerSliceRef cpb)
{
	(void) rpf;
	(void) cpf;
	const idx_t m = (idx_t) L.nrows, n = (idx_t) U.ncols;
	const idx_t size = m < n ? m : n;
	FH_CHECK((idx_t) Out.nrows == m && (idx_t) Out.ncols == n && (idx_t) L.ncols >= size && (idx_t) U.nrows >= size,
		 "full_piv_lu reconstruct: dimension mismatch");
	DevPerm rows("full_piv_lu reconstruct", rpb, m, I{}), cols("full_piv_lu reconstruct", cpb, n, I{});
	if (m == 0 || n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> o(view<T>(Out), false, true);
	Scratch tb((size_t) m * (size_t) n * sizeof(T));
	MatV<T> tmp{tb.as<T>(), m, n, 1, m};
	matmul_triangular_dev<T>(tmp.sub(0, 0, size, size), 0, false, l.dev.sub(0, 0, size, size), 5, u.dev.sub(0, 0, size, size), 2, (T) 1);
	if (m > n)
		matmul_triangular_dev<T>(tmp.sub(size, 0, m - size, size), 0, false, l.dev.sub(size, 0, m - size, size), 0, u.dev.sub(0, 0, size, size), 2,
					 (T) 1);
	if (m < n)
		matmul_triangular_dev<T>(tmp.sub(0, size, size, n - size), 0, false, l.dev.sub(0, 0, size, size), 5, u.dev.sub(0, size, size, n - size), 0,
					 (T) 1);
	gather_rows_cols<T>(o.dev, tmp, rows, cols);
	ctx().sync();
}

// lu/full_pivoting/inverse.rs: out(i, j) = (U^-1 L^-1)(col_perm_inv[i], row_perm_inv[j])
template <typename T, typename I>
void full_lu_inverse_api(FaerMatMut Out, FaerMatRef L, FaerMatRef U, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf, FaerSliceRef cpb)
{
	(void) rpf;
	(void) cpf;
	const idx_t n = (idx_t) L.ncols;
	FH_CHECK((idx_t) L.nrows == n && (idx_t) U.nrows == n && (idx_t) U.ncols == n && (idx_t) Out.nrows == n && (idx_t) Out.ncols == n,
		 "full_piv_lu inverse: dimension mismatch");
	DevPerm rows("full_piv_lu inverse", cpb, n, I{}), cols("full_piv_lu inverse", rpb, n, I{});
	if (n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), u(view<T>(U), true, false);
	Staged<T> o(view<T>(Out), false, true);
	Scratch tb((size_t) n * (size_t) n * sizeof(T));
	MatV<T> tmp{tb.as<T>(), n, n, 1, n};
	tri_invert_lower_dev<T>(o.dev, l.dev, true);
	tri_invert_lower_dev<T>(o.dev.t(), u.dev.t(), false);
	matmul_triangular_dev<T>(tmp, 0, false, o.dev.c(), 2, o.dev.c(), 5, (T) 1);
	gather_rows_cols<T>(o.dev, tmp, rows, cols);
	ctx().sync();
}

// qr/col_pivoting/reconstruct.rs: (Q R) with its columns permuted back; inverse.rs: rows of R^-1 Q^H permuted back
template <typename T, typename I>
void colpiv_qr_reconstruct_api(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerSliceRef pf, FaerSliceRef pb)
{
	(void) pf;
	qr_reconstruct_check(Out, Qb, Qc, R);
	DevPerm perm_bwd("colpiv_qr reconstruct", pb, (idx_t) R.ncols, I{});
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> o(view<T>(Out), false, true);
	qr_reconstruct_dev<T>(o.dev, f.qb.dev, f.qc.dev, f.r.dev);
	permute_rows<T>(o.dev.t(), perm_bwd); // permute_cols_in_place(out, col_perm.inverse())
}
template <typename T, typename I>
void colpiv_qr_inverse_api(FaerMatMut Out, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerSliceRef pf, FaerSliceRef pb)
{
	(void) pf;
	qr_inverse_check(Out, Qb, Qc, R);
	DevPerm perm_bwd("colpiv_qr inverse", pb, (idx_t) R.ncols, I{});
	QrFactors<T> f(Qb, Qc, R);
	Staged<T> o(view<T>(Out), false, true);
	qr_inverse_dev<T>(o.dev, f.qb.dev, f.qc.dev, f.r.dev);
	permute_rows<T>(o.dev, perm_bwd); // permute_rows_in_place(out, col_perm.inverse())
}

// evd/mod.rs:270-425 behind lib.rs:2385-2399 (U.ncols == 0: no eigenvectors)
// evd/mod.rs:1213 evd_real.  All device memory of the call -- the working matrices of evd_dev and the staged images of host
// operands -- is one arena (arena.h).
template <typename T> FaerEvdStatus evd_api(FaerMatRef A, FaerMatMut UL, FaerMatMut UR, FaerVecMut S, FaerVecMut S_im, FaerEvdParams params)
{
	const size_t n = A.nrows;
	FH_CHECK(A.ncols == n && S.len == n && S_im.len == n, "evd: A must be square, S and S_im must have n entries"); // mod.rs:1224
	FH_CHECK(UL.ncols == 0 || (UL.nrows == n && UL.ncols == n), "evd: UL must be n x n (or have no columns)");
	FH_CHECK(UR.ncols == 0 || (UR.nrows == n && UR.ncols == n), "evd: UR must be n x n (or have no columns)");
	FH_CHECK(params.schur.recommended_shift_count != nullptr, "evd: params.schur.recommended_shift_count is NULL");
	FaerEvdStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerEvdStatus_Ok;
	if (n == 0)
		return st; // mod.rs:1018
	ctx().ensure_device();
	const bool want_l = UL.ncols != 0, want_r = UR.ncols != 0;
	const idx_t N = (idx_t) n, bs = (idx_t) qr_block_size(n - 1, n - 1);
	const MatV<const T> a = view<T>(A);
	const MatV<T> ul = view<T>(UL), ur = view<T>(UR), s = vview<T>(S), si = vview<T>(S_im);
	const bool a_host = !is_device_ptr(a.p), ul_host = want_l && !is_device_ptr(ul.p), ur_host = want_r && !is_device_ptr(ur.p);
	const size_t nn = Arena::padded(n * n * sizeof(T));
	int r;
	{
		Arena ar(evd_arena_bytes(N, want_l || want_r, bs < 1 ? 1 : bs, (int) sizeof(T)) + (size_t) ul_host * nn + (size_t) ur_host * nn + 512);
		T *wr = ar.take<T>(n), *wi = ar.take<T>(n);
		const MatV<T> dl = ul_host ? ar.mat<T>(N, N) : (want_l ? ul : MatV<T>{nullptr, N, N, 1, N});
		const MatV<T> dr = ur_host ? ar.mat<T>(N, N) : (want_r ? ur : MatV<T>{nullptr, N, N, 1, N});
		const MatV<const T> da = a_host ? ar.copy_in<T>(a).c() : a;
		r = evd_dev<T>(ar, da, a_host, dl, dr, wr, wi, bs < 1 ? 1 : bs, params.schur.recommended_shift_count);
		if (r == 0) {
			const MatV<const T> wrv{wr, N, 1, 1, N}, wiv{wi, N, 1, 1, N};
			if (is_device_ptr(s.p))
				copy_dev<T>(s, wrv);
			else
				Arena::copy_out<T>(s, wrv);
			if (is_device_ptr(si.p))
				copy_dev<T>(si, wiv);
			else
				Arena::copy_out<T>(si, wiv);
			if (ul_host)
				Arena::copy_out<T>(ul, dl.c());
			if (ur_host)
				Arena::copy_out<T>(ur, dr.c());
			ctx().sync();
		}
	}
	st.tag = r == 0 ? FaerEvdStatus_Ok : FaerEvdStatus_NoConvergence;
	return st;
}

// gevd/mod.rs:130-320 behind lib.rs:2459-2520 (U.ncols == 0: no eigenvectors).  One arena holds the working matrices of gevd_dev,
// the three eigenvalue vectors and the staged images of host operands.
template <typename T>
FaerGevdStatus gevd_api(FaerMatMut Am, FaerMatMut Bm, FaerMatMut UL, FaerMatMut UR, FaerVecMut Al, FaerVecMut Ai, FaerVecMut Be, FaerGevdParams params)
{
	const size_t n = Am.nrows;
	FH_CHECK(params.schur.recommended_shift_count != nullptr, "generalized_evd: params.schur.recommended_shift_count is NULL");
	FH_CHECK(Am.ncols == n && Bm.nrows == n && Bm.ncols == n, "generalized_evd: A and B must be square and of one size");
	FH_CHECK(Al.len == n && Ai.len == n && Be.len == n, "generalized_evd: alpha, alpha_im and beta must have n entries");
	FH_CHECK(UL.ncols == 0 || (UL.nrows == n && UL.ncols == n), "generalized_evd: UL must be n x n (or have no columns)");
	FH_CHECK(UR.ncols == 0 || (UR.nrows == n && UR.ncols == n), "generalized_evd: UR must be n x n (or have no columns)");
	FaerGevdStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerGevdStatus_Ok;
	if (n == 0)
		return st; // mod.rs:183
	ctx().ensure_device();
	const bool want_l = UL.ncols != 0, want_r = UR.ncols != 0;
	const idx_t N = (idx_t) n, bs0 = (idx_t) qr_block_size(n, n), bs = bs0 < 1 ? 1 : bs0;
	const FaerMatRef Ar{Am.ptr, Am.nrows, Am.ncols, Am.row_stride, Am.col_stride}, Br{Bm.ptr, Bm.nrows, Bm.ncols, Bm.row_stride, Bm.col_stride};
	const MatV<const T> a = view<T>(Ar), b = view<T>(Br);
	const MatV<T> ul = view<T>(UL), ur = view<T>(UR), outs[3] = {vview<T>(Al), vview<T>(Ai), vview<T>(Be)};
	const bool a_host = !is_device_ptr(a.p), b_host = !is_device_ptr(b.p), ul_host = want_l && !is_device_ptr(ul.p), ur_host = want_r && !is_device_ptr(ur.p);
	const size_t nn = Arena::padded(n * n * sizeof(T));
	int r;
	{
		Arena ar(gevd_arena_bytes(N, want_l || want_r, bs, (int) sizeof(T)) + 3 * Arena::padded(n * sizeof(T))
			 + ((size_t) a_host + (size_t) b_host + (size_t) ul_host + (size_t) ur_host) * nn + 512);
		T *ev[3] = {ar.take<T>(n), ar.take<T>(n), ar.take<T>(n)};
		const MatV<T> dl = ul_host ? ar.mat<T>(N, N) : (want_l ? ul : MatV<T>{nullptr, N, N, 1, N});
		const MatV<T> dr = ur_host ? ar.mat<T>(N, N) : (want_r ? ur : MatV<T>{nullptr, N, N, 1, N});
		const MatV<const T> da = a_host ? ar.copy_in<T>(a).c() : a, db = b_host ? ar.copy_in<T>(b).c() : b;
		r = gevd_dev<T>(ar, da, db, dl, dr, ev[0], ev[1], ev[2], bs, (idx_t) 48 * 48, params.schur.recommended_shift_count);
		if (r != 0) { // mod.rs:225-234 (and the same outputs where the iteration cap is reached)
			const T nan = std::numeric_limits<T>::quiet_NaN();
			for (int k = 0; k < 3; ++k)
				fill_dev<T>(MatV<T>{ev[k], N, 1, 1, N}, DST_FULL, nan);
			if (want_l)
				fill_dev<T>(dl, DST_FULL, nan);
			if (want_r)
				fill_dev<T>(dr, DST_FULL, nan);
		}
		for (int k = 0; k < 3; ++k) {
			const MatV<const T> src{ev[k], N, 1, 1, N};
			if (is_device_ptr(outs[k].p))
				copy_dev<T>(outs[k], src);
			else
				Arena::copy_out<T>(outs[k], src);
		}
		if (ul_host)
			Arena::copy_out<T>(ul, dl.c());
		if (ur_host)
			Arena::copy_out<T>(ur, dr.c());
		ctx().sync();
	}
	st.tag = r == 0 ? FaerGevdStatus_Ok : FaerGevdStatus_NoConvergence;
	return st;
}

// cholesky/llt/update.rs:360-379 and cholesky/ldlt/update.rs:376-400
template <typename T> FaerLltStatus chol_update_api(FaerMatMut L, FaerMatMut W, FaerVecMut alpha, bool ldlt)
{
	const size_t n = L.nrows, r = W.ncols;
	FH_CHECK(L.ncols == n && W.nrows == n && alpha.len == r, "rank_r_update: L must be n x n, W n x r, alpha must have r entries");
	FaerLltStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerLltStatus_Ok;
	if (n == 0 || r == 0)
		return st;
	ctx().ensure_device();
	const long res = chol_rank_update<T>(view<T>(L), view<T>(W), vview<T>(alpha), ldlt);
	if (res >= 0) {
		st.tag = FaerLltStatus_NonPositivePivot;
		st.non_positive_pivot.index = (size_t) res;
	}
	return st;
}

// cholesky/ldlt/update.rs:417-434: the indices are sorted in place, then checked
template <typename T, typename I> void ldlt_delete_api(FaerMatMut LD, FaerSliceMut indices)
{
	const size_t n = LD.nrows, r = indices.len;
	FH_CHECK(LD.ncols == n, "delete_rows_and_cols: LD must be square");
	if (r == 0)
		return;
	FH_CHECK(indices.ptr != nullptr && !is_device_ptr(indices.ptr), "delete_rows_and_cols: the index slice must be host memory");
	I *ip = static_cast<I *>(indices.ptr);
	std::sort(ip, ip + r);
	std::vector<idx_t> idx(r);
	for (size_t k = 0; k < r; ++k) {
		FH_CHECK(k == 0 || ip[k] > ip[k - 1], "delete_rows_and_cols: an index is listed twice");
		idx[k] = (idx_t) ip[k];
	}
	FH_CHECK((size_t) ip[r - 1] < n, "delete_rows_and_cols: an index is out of bounds");
	ctx().ensure_device();
	ldlt_delete_rows_and_cols<T>(view<T>(LD), idx.data(), (idx_t) r);
}

template <typename T> FaerEvdStatus self_adjoint_evd_api(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerSelfAdjointEvdParams params)
{
	const size_t n = A.nrows;
	FH_CHECK(A.ncols == n && S.len == n, "self_adjoint_evd: A must be square and S must have n entries"); // mod.rs:279
	FH_CHECK(U.ncols == 0 || (U.nrows == n && U.ncols == n), "self_adjoint_evd: U must be n x n (or have no columns)");
	FaerEvdStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerEvdStatus_Ok;
	if (n == 0)
		return st;
	int r;
	{
		Staged<const T> a(view<T>(A), true, false);
		FaerMatMut Sm{S.ptr, S.len, 1, S.stride, 0};
		Staged<T> s(view<T>(Sm), false, true);
		const idx_t leaf = evd_leaf_size(params.recursion_threshold), bs = (idx_t) qr_block_size(n, n);
		if (U.ncols == 0) {
			r = self_adjoint_evd_dev<T>(a.dev, MatV<T>{nullptr, (idx_t) n, (idx_t) n, 1, (idx_t) n}, s.dev.p, s.dev.rs, leaf, bs);
		} else {
			Staged<T> u(view<T>(U), false, true);
			r = self_adjoint_evd_dev<T>(a.dev, u.dev, s.dev.p, s.dev.rs, leaf, bs);
		}
	}
	if (r != 0)
		st.tag = FaerEvdStatus_NoConvergence;
	return st;
}

// svd/mod.rs:530-671 behind lib.rs:2327-2366 (U.ncols == 0 / V.ncols == 0: no left / right vectors)
template <typename T> FaerSvdStatus svd_api(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerMatMut V, FaerSvdParams params)
{
	const size_t m = A.nrows, n = A.ncols, size = m < n ? m : n;
	FH_CHECK(S.len == size, "svd: S must have min(nrows, ncols) entries"); // mod.rs:542
	FH_CHECK(U.ncols == 0 || (U.nrows == m && (U.ncols == m || U.ncols == size)), "svd: U must be nrows x min(nrows, ncols) or nrows x nrows");
	FH_CHECK(V.ncols == 0 || (V.nrows == n && (V.ncols == n || V.ncols == size)), "svd: V must be ncols x min(nrows, ncols) or ncols x ncols");
	FaerSvdStatus st;
	memset(&st, 0, sizeof(st));
	st.tag = FaerSvdStatus_Ok;
	if (size == 0) {
		// mod.rs:586-591: the left factor of the (transposed) problem is the identity pattern, the other one has no entries
		FaerMatMut I = n > m ? V : U;
		if (I.ncols > 0 && I.nrows > 0) {
			Staged<T> e(view<T>(I), false, true);
			svd_identity_dev<T>(e.dev);
			ctx().sync();
		}
		return st;
	}
	int r;
	{
		Staged<const T> a(view<T>(A), true, false);
		FaerMatMut Sm{S.ptr, S.len, 1, S.stride, 0};
		Staged<T> s(view<T>(Sm), false, true);
		FaerMatMut none{nullptr, 0, 0, 0, 0};
		Staged<T> u(view<T>(U.ncols ? U : none), false, true), v(view<T>(V.ncols ? V : none), false, true);
		MatV<T> ud = u.dev, vd = v.dev;
		if (U.ncols == 0)
			ud = MatV<T>{nullptr, (idx_t) m, 0, 1, (idx_t) m};
		if (V.ncols == 0)
			vd = MatV<T>{nullptr, (idx_t) n, 0, 1, (idx_t) n};
		const size_t big = m < n ? n : m;
		r = svd_dev<T>(a.dev, ud, vd, s.dev.p, s.dev.rs, svd_leaf_size(params.recursion_threshold), params.qr_ratio_threshold,
			       (idx_t) params.qr.blocking_threshold, (idx_t) qr_block_size(big, size), (idx_t) qr_block_size(size, size));
	}
	if (r != 0)
		st.tag = FaerSvdStatus_NoConvergence;
	return st;
}

} // namespace

extern "C" {

// ---------------------------------------------------------------------------------------- inner boundary
void faer_hip_gemm(FaerHipDType dtype, FaerHipIType itype, size_t m, size_t n, size_t k, void *dst, ptrdiff_t dst_rs,
		   ptrdiff_t dst_cs, const void *row_idx, const void *col_idx, FaerHipDstKind dst_kind, FaerAccum accum,
		   const void *lhs, ptrdiff_t lhs_rs, ptrdiff_t lhs_cs, bool conj_lhs, const void *diag, ptrdiff_t diag_stride,
		   const void *rhs, ptrdiff_t rhs_rs, ptrdiff_t rhs_cs, bool conj_rhs, const void *alpha, size_t n_threads)
{
	(void) n_threads;
	const bool cx = dtype == FaerHipDType_C32 || dtype == FaerHipDType_C64;
	FH_CHECK(cx || dtype == FaerHipDType_F32 || dtype == FaerHipDType_F64, "faer_hip_gemm: unknown dtype");
	FH_CHECK(!cx || (!row_idx && !col_idx && !diag),
		 "faer_hip_gemm: row_idx / col_idx / diag are not implemented for complex scalars (c32 / c64)");
	FH_CHECK(alpha != nullptr, "faer_hip_gemm: alpha is NULL");
	if (m == 0 || n == 0)
		return;
	const bool add = accum == FaerAccum_Add;
	auto run = [&](auto tag) {
		typedef decltype(tag) T;
		const size_t isz = itype == FaerHipIType_U64 ? 8 : 4;
		// extent of dst in rows / cols when scattered through the index arrays
		idx_t drows = (idx_t) m, dcols = (idx_t) n;
		std::vector<unsigned char> hri, hci;
		auto max_idx = [&](const void *p, size_t cnt) {
			idx_t mx = 0;
			for (size_t i = 0; i < cnt; ++i) {
				idx_t v = isz == 8 ? (idx_t) static_cast<const uint64_t *>(p)[i]
						   : (idx_t) static_cast<const uint32_t *>(p)[i];
				if (v > mx)
					mx = v;
			}
			return mx;
		};
		const bool ri_host = row_idx && !is_device_ptr(row_idx), ci_host = col_idx && !is_device_ptr(col_idx);
		FH_CHECK((!row_idx || ri_host || is_device_ptr(dst)) && (!col_idx || ci_host || is_device_ptr(dst)),
			 "faer_hip_gemm: device index arrays require a device dst");
		if (ri_host)
			drows = max_idx(row_idx, m) + 1;
		if (ci_host)
			dcols = max_idx(col_idx, n) + 1;
		MatV<T> D{static_cast<T *>(dst), drows, dcols, (idx_t) dst_rs, (idx_t) dst_cs};
		MatV<const T> A{static_cast<const T *>(lhs), (idx_t) m, (idx_t) k, (idx_t) lhs_rs, (idx_t) lhs_cs};
		MatV<const T> B{static_cast<const T *>(rhs), (idx_t) k, (idx_t) n, (idx_t) rhs_rs, (idx_t) rhs_cs};
		MatV<const T> Dg{static_cast<const T *>(diag), diag ? (idx_t) k : 0, 1, (idx_t) diag_stride, 0};
		Staged<const T> a(A, true, false), b(B, true, false), dg(Dg, true, false);
		// a non-Full or scattered dst keeps untouched entries => copy in
		Staged<T> c(D, add || dst_kind != FaerHipDstKind_Full || row_idx || col_idx, true);
		Staged<const unsigned char> ri(MatV<const unsigned char>{static_cast<const unsigned char *>(row_idx),
									  row_idx ? (idx_t) (m * isz) : 0, 1, 1, 0},
					       true, false);
		Staged<const unsigned char> ci(MatV<const unsigned char>{static_cast<const unsigned char *>(col_idx),
									  col_idx ? (idx_t) (n * isz) : 0, 1, 1, 0},
					       true, false);
		GemmExtra<T> ex;
		ex.row_idx = row_idx ? ri.dev.p : nullptr;
		ex.col_idx = col_idx ? ci.dev.p : nullptr;
		ex.idx64 = isz == 8;
		ex.diag = diag ? dg.dev.p : nullptr;
		ex.diag_stride = dg.dev.rs; // 1 for a staged host vector, the caller's stride for a device one
		ex.conj_lhs = conj_lhs;	    // (the real kernels never look: conjugation is the identity there)
		ex.conj_rhs = conj_rhs;
		MatV<T> Cv{c.dev.p, (idx_t) m, (idx_t) n, c.dev.rs, c.dev.cs};
		gemm_dev<T>(Cv, (DstKind) dst_kind, add, a.dev, b.dev, *static_cast<const T *>(alpha), &ex);
	};
	if (dtype == FaerHipDType_F64)
		run(double());
	else if (dtype == FaerHipDType_F32)
		run(float());
	else if (dtype == FaerHipDType_C64)
		run(c64());
	else
		run(c32());
}

// ---------------------------------------------------------------------------------------- outer boundary
// One short macro per family: defined, expanded over exactly the lists the family supports, undefined again.  Every wrapper is
// checked against its prototype in include/faer_hip.h.  An argument that the device path does not use (par, mem, most params;
// conj where a family is real only) is left unnamed.  Adding a scalar type to a family = adding it to that family's list.
//
// scalar lists: X(suf, T)
#define FH_FOR_REAL(X) X(f64, double) X(f32, float)
#define FH_FOR_COMPLEX(X) X(c64, c64) X(c32, c32)
#define FH_FOR_SCALARS(X) FH_FOR_REAL(X) FH_FOR_COMPLEX(X)
#define FH_FOR_DTYPES(X) FH_FOR_REAL(X)
// index list: X(suf, T, it, I).  FH_FOR_INDEXED(LIST) expands the family's X over a scalar list times the index list.
#define FH_FOR_INDICES(X, suf, T) X(suf, T, u32, uint32_t) X(suf, T, u64, uint64_t)
#define FH_X_PER_INDEX(suf, T) FH_FOR_INDICES(X, suf, T)
#define FH_FOR_INDEXED(LIST) LIST(FH_X_PER_INDEX)

// level 3 (faer-ffi/src/lib.rs:855-937), real and complex: the triangular solves honour their FaerConj (the identity for a real T)
#define X(suf, T)                                                                                                      \
	void libfaer_v0_23_matmul_##suf(FaerMatMut C, FaerAccum accum, FaerMatRef A, FaerMatRef B, const void *alpha,  \
					FaerPar)                                                                       \
	{                                                                                                              \
		matmul_api<T>(C, accum, A, B, alpha);                                                                  \
	}                                                                                                              \
	void libfaer_v0_23_matmul_triangular_##suf(FaerMatMut C, FaerBlock C_block, FaerAccum accum, FaerMatRef A,     \
						   FaerBlock A_block, FaerMatRef B, FaerBlock B_block,                 \
						   const void *alpha, FaerPar)                                         \
	{                                                                                                              \
		matmul_triangular_api<T>(C, C_block, accum, A, A_block, B, B_block, alpha);                            \
	}                                                                                                              \
	void libfaer_v0_23_solve_triangular_lower_in_place_##suf(FaerMatRef L, FaerConj cj, FaerMatMut rhs, FaerPar)   \
	{                                                                                                              \
		trsm_api<T>(L, rhs, false, false, cj == FaerConj_Yes);                                                 \
	}                                                                                                              \
	void libfaer_v0_23_solve_triangular_upper_in_place_##suf(FaerMatRef U, FaerConj cj, FaerMatMut rhs, FaerPar)   \
	{                                                                                                              \
		trsm_api<T>(U, rhs, true, false, cj == FaerConj_Yes);                                                  \
	}                                                                                                              \
	void libfaer_v0_23_solve_unit_triangular_lower_in_place_##suf(FaerMatRef L, FaerConj cj, FaerMatMut rhs,       \
								      FaerPar)                                         \
	{                                                                                                              \
		trsm_api<T>(L, rhs, false, true, cj == FaerConj_Yes);                                                  \
	}                                                                                                              \
	void libfaer_v0_23_solve_unit_triangular_upper_in_place_##suf(FaerMatRef U, FaerConj cj, FaerMatMut rhs,       \
								      FaerPar)                                         \
	{                                                                                                              \
		trsm_api<T>(U, rhs, true, true, cj == FaerConj_Yes);                                                   \
	}
FH_FOR_SCALARS(X)
#undef X

// triangular inverse (lib.rs:938-983)
#define X(suf, T)                                                                                                      \
	void libfaer_v0_23_inverse_triangular_lower_in_place_##suf(FaerMatMut T_inv, FaerMatRef Tm, FaerPar)           \
	{                                                                                                              \
		tri_inverse_api<T>(T_inv, Tm, false, false);                                                           \
	}                                                                                                              \
	void libfaer_v0_23_inverse_triangular_upper_in_place_##suf(FaerMatMut T_inv, FaerMatRef Tm, FaerPar)           \
	{                                                                                                              \
		tri_inverse_api<T>(T_inv, Tm, true, false);                                                            \
	}                                                                                                              \
	void libfaer_v0_23_inverse_unit_triangular_lower_in_place_##suf(FaerMatMut T_inv, FaerMatRef Tm, FaerPar)      \
	{                                                                                                              \
		tri_inverse_api<T>(T_inv, Tm, false, true);                                                            \
	}                                                                                                              \
	void libfaer_v0_23_inverse_unit_triangular_upper_in_place_##suf(FaerMatMut T_inv, FaerMatRef Tm, FaerPar)      \
	{                                                                                                              \
		tri_inverse_api<T>(T_inv, Tm, true, true);                                                             \
	}
FH_FOR_SCALARS(X)
#undef X

// LLT (lib.rs:650-655 params, :984-1040 factor and solve, :1039-1075 reconstruct and inverse)
#define X(suf, T)                                                                                                      \
	FaerLltParams libfaer_v0_23_LltParams_##suf(void) { return FaerLltParams{64, 128}; }                           \
	FaerLayout libfaer_v0_23_llt_factor_in_place_scratch_##suf(size_t dim, FaerPar, FaerLltParams)                 \
	{                                                                                                              \
		return layout(dim * sizeof(T), 64);                                                                    \
	}                                                                                                              \
	FaerLltStatus libfaer_v0_23_llt_factor_in_place_##suf(FaerMatMut A, FaerLltRegularization reg, FaerPar,        \
							      FaerMemAlloc, FaerLltParams)                             \
	{                                                                                                              \
		return llt_api<T>(A, reg);                                                                             \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_llt_solve_in_place_scratch_##suf(size_t, size_t, FaerPar) { return layout(0, 1); }    \
	void libfaer_v0_23_llt_solve_in_place_##suf(FaerMatRef L, FaerConj, FaerMatMut rhs, FaerPar, FaerMemAlloc)     \
	{                                                                                                              \
		llt_solve_api<T>(L, rhs);                                                                              \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_llt_reconstruct_scratch_##suf(size_t, FaerPar) { return layout(0, 1); }               \
	void libfaer_v0_23_llt_reconstruct_##suf(FaerMatMut A, FaerMatRef L, FaerPar, FaerMemAlloc)                    \
	{                                                                                                              \
		llt_reconstruct_api<T>(A, L);                                                                          \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_llt_inverse_scratch_##suf(size_t dim, FaerPar)                                        \
	{                                                                                                              \
		return layout(dim * dim * sizeof(T), 64);                                                              \
	}                                                                                                              \
	void libfaer_v0_23_llt_inverse_##suf(FaerMatMut A_inv, FaerMatRef L, FaerPar, FaerMemAlloc)                    \
	{                                                                                                              \
		llt_inverse_api<T>(A_inv, L);                                                                          \
	}
FH_FOR_REAL(X)
#undef X

// LDLT (lib.rs:660-664 params, :1189-1250 factor and solve, :1247-1288 reconstruct and inverse)
#define X(suf, T)                                                                                                      \
	FaerLdltParams libfaer_v0_23_LdltParams_##suf(void) { return FaerLdltParams{64, 128}; }                        \
	FaerLayout libfaer_v0_23_ldlt_factor_in_place_scratch_##suf(size_t dim, FaerPar, FaerLdltParams)               \
	{                                                                                                              \
		return layout(dim * sizeof(T), 64);                                                                    \
	}                                                                                                              \
	FaerLdltStatus libfaer_v0_23_ldlt_factor_in_place_##suf(FaerMatMut A, FaerLdltRegularization reg, FaerPar,     \
								FaerMemAlloc, FaerLdltParams)                          \
	{                                                                                                              \
		return ldlt_api<T>(A, reg);                                                                            \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_ldlt_solve_in_place_scratch_##suf(size_t, size_t, FaerPar) { return layout(0, 1); }   \
	void libfaer_v0_23_ldlt_solve_in_place_##suf(FaerMatRef L, FaerVecRef D, FaerConj, FaerMatMut rhs, FaerPar,    \
						     FaerMemAlloc)                                                     \
	{                                                                                                              \
		ldlt_solve_api<T>(L, D, rhs);                                                                          \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_ldlt_reconstruct_scratch_##suf(size_t dim, FaerPar)                                   \
	{                                                                                                              \
		return layout(dim * dim * sizeof(T), 64);                                                              \
	}                                                                                                              \
	void libfaer_v0_23_ldlt_reconstruct_##suf(FaerMatMut A, FaerMatRef L, FaerVecRef D, FaerPar, FaerMemAlloc)     \
	{                                                                                                              \
		ldlt_reconstruct_api<T>(A, L, D);                                                                      \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_ldlt_inverse_scratch_##suf(size_t dim, FaerPar)                                       \
	{                                                                                                              \
		return layout(dim * dim * sizeof(T), 64);                                                              \
	}                                                                                                              \
	void libfaer_v0_23_ldlt_inverse_##suf(FaerMatMut A_inv, FaerMatRef L, FaerVecRef D, FaerPar, FaerMemAlloc)     \
	{                                                                                                              \
		ldlt_inverse_api<T>(A_inv, L, D);                                                                      \
	}
FH_FOR_REAL(X)
#undef X

// partial-pivot LU, real and complex (lib.rs:679-685 params, :1952-1984 factor, :1985-2056 solves): the solves honour A_conj.
// The scratch queries are the reference's: min(dim, block_size) indices for the factorization, one copy of rhs for a solve.
#define X(suf, T)                                                                                                      \
	FaerPartialPivLuParams libfaer_v0_23_PartialPivLuParams_##suf(void)                                            \
	{                                                                                                              \
		return FaerPartialPivLuParams{16, 64, 128 * 128};                                                      \
	}
FH_FOR_SCALARS(X)
#undef X
#define X(suf, T, it, I)                                                                                               \
	FaerLayout libfaer_v0_23_partial_piv_lu_factor_in_place_scratch_##it##_##suf(size_t dim, size_t bs, FaerPar,   \
										      FaerPartialPivLuParams)          \
	{                                                                                                              \
		return layout((dim < bs ? dim : bs) * sizeof(I), sizeof(I));                                           \
	}                                                                                                              \
	FaerPartialPivLuStatus libfaer_v0_23_partial_piv_lu_factor_in_place_##it##_##suf(                              \
		FaerMatMut A, FaerSliceMut pf, FaerSliceMut pb, FaerPar, FaerMemAlloc, FaerPartialPivLuParams)         \
	{                                                                                                              \
		return lu_api<T, I>(A, pf, pb);                                                                        \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_partial_piv_lu_solve_in_place_scratch_##it##_##suf(size_t dim, size_t k, FaerPar)     \
	{                                                                                                              \
		return layout(dim * k * sizeof(T), 64);                                                                \
	}                                                                                                              \
	void libfaer_v0_23_partial_piv_lu_solve_in_place_##it##_##suf(                                                 \
		FaerMatRef L, FaerMatRef U, FaerConj cj, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs, FaerPar,    \
		FaerMemAlloc)                                                                                          \
	{                                                                                                              \
		lu_solve_api<T, I>(L, U, pf, pb, rhs, false, cj == FaerConj_Yes);                                      \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_scratch_##it##_##suf(size_t dim, size_t k,    \
											       FaerPar)                \
	{                                                                                                              \
		return layout(dim * k * sizeof(T), 64);                                                                \
	}                                                                                                              \
	void libfaer_v0_23_partial_piv_lu_solve_transpose_in_place_##it##_##suf(                                       \
		FaerMatRef L, FaerMatRef U, FaerConj cj, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs, FaerPar,    \
		FaerMemAlloc)                                                                                          \
	{                                                                                                              \
		lu_solve_api<T, I>(L, U, pf, pb, rhs, true, cj == FaerConj_Yes);                                       \
	}
FH_FOR_INDEXED(FH_FOR_SCALARS)
#undef X
// reconstruct and inverse (lib.rs:2071-2124) are real only: the header declares no complex prototype for them
#define X(suf, T, it, I)                                                                                               \
	FaerLayout libfaer_v0_23_partial_piv_lu_reconstruct_scratch_##it##_##suf(size_t nrows, size_t ncols, FaerPar)  \
	{                                                                                                              \
		return layout(nrows * ncols * sizeof(T), 64);                                                          \
	}                                                                                                              \
	void libfaer_v0_23_partial_piv_lu_reconstruct_##it##_##suf(                                                    \
		FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef pf, FaerSliceRef pb, FaerPar, FaerMemAlloc)     \
	{                                                                                                              \
		lu_reconstruct_api<T, I>(A, L, U, pf, pb);                                                             \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_partial_piv_lu_inverse_scratch_##it##_##suf(size_t dim, FaerPar)                      \
	{                                                                                                              \
		return layout(dim * dim * sizeof(T), 64);                                                              \
	}                                                                                                              \
	void libfaer_v0_23_partial_piv_lu_inverse_##it##_##suf(                                                        \
		FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef pf, FaerSliceRef pb, FaerPar, FaerMemAlloc) \
	{                                                                                                              \
		lu_inverse_api<T, I>(A_inv, L, U, pf, pb);                                                             \
	}
FH_FOR_INDEXED(FH_FOR_REAL)
#undef X

// full-pivot LU (lib.rs:2125-2260 factor and solves, :2246-2330 reconstruct and inverse)
#define X(suf, T)                                                                                                      \
	FaerFullPivLuParams libfaer_v0_23_FullPivLuParams_##suf(void) { return FaerFullPivLuParams{256 * 512}; }
FH_FOR_REAL(X)
#undef X
#define X(suf, T, it, I)                                                                                               \
	FaerLayout libfaer_v0_23_full_piv_lu_factor_in_place_scratch_##it##_##suf(size_t dim, size_t, FaerPar,         \
										   FaerFullPivLuParams)                \
	{                                                                                                              \
		return layout(dim * 2 * sizeof(size_t), sizeof(size_t));                                               \
	}                                                                                                              \
	FaerFullPivLuStatus libfaer_v0_23_full_piv_lu_factor_in_place_##it##_##suf(                                    \
		FaerMatMut A, FaerSliceMut rpf, FaerSliceMut rpb, FaerSliceMut cpf, FaerSliceMut cpb, FaerPar,         \
		FaerMemAlloc, FaerFullPivLuParams)                                                                     \
	{                                                                                                              \
		return full_lu_api<T, I>(A, rpf, rpb, cpf, cpb);                                                       \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_full_piv_lu_solve_in_place_scratch_##it##_##suf(size_t dim, size_t k, FaerPar)        \
	{                                                                                                              \
		return layout(dim * k * sizeof(T), 64);                                                                \
	}                                                                                                              \
	void libfaer_v0_23_full_piv_lu_solve_in_place_##it##_##suf(                                                    \
		FaerMatRef L, FaerMatRef U, FaerConj, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf,            \
		FaerSliceRef cpb, FaerMatMut rhs, FaerPar, FaerMemAlloc)                                               \
	{                                                                                                              \
		full_lu_solve_api<T, I>(L, U, rpf, rpb, cpf, cpb, rhs, false);                                         \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_full_piv_lu_solve_transpose_in_place_scratch_##it##_##suf(size_t dim, size_t k,       \
											    FaerPar)                   \
	{                                                                                                              \
		return layout(dim * k * sizeof(T), 64);                                                                \
	}                                                                                                              \
	void libfaer_v0_23_full_piv_lu_solve_transpose_in_place_##it##_##suf(                                          \
		FaerMatRef L, FaerMatRef U, FaerConj, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf,            \
		FaerSliceRef cpb, FaerMatMut rhs, FaerPar, FaerMemAlloc)                                               \
	{                                                                                                              \
		full_lu_solve_api<T, I>(L, U, rpf, rpb, cpf, cpb, rhs, true);                                          \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_full_piv_lu_reconstruct_scratch_##it##_##suf(size_t nrows, size_t ncols, FaerPar)     \
	{                                                                                                              \
		return layout(nrows * ncols * sizeof(T), 64);                                                          \
	}                                                                                                              \
	void libfaer_v0_23_full_piv_lu_reconstruct_##it##_##suf(                                                       \
		FaerMatMut A, FaerMatRef L, FaerMatRef U, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf,        \
		FaerSliceRef cpb, FaerPar, FaerMemAlloc)                                                               \
	{                                                                                                              \
		full_lu_reconstruct_api<T, I>(A, L, U, rpf, rpb, cpf, cpb);                                            \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_full_piv_lu_inverse_scratch_##it##_##suf(size_t dim, FaerPar)                         \
	{                                                                                                              \
		return layout(dim * dim * sizeof(T), 64);                                                              \
	}                                                                                                              \
	void libfaer_v0_23_full_piv_lu_inverse_##it##_##suf(                                                           \
		FaerMatMut A_inv, FaerMatRef L, FaerMatRef U, FaerSliceRef rpf, FaerSliceRef rpb, FaerSliceRef cpf,    \
		FaerSliceRef cpb, FaerPar, FaerMemAlloc)                                                               \
	{                                                                                                              \
		full_lu_inverse_api<T, I>(A_inv, L, U, rpf, rpb, cpf, cpb);                                            \
	}
FH_FOR_INDEXED(FH_FOR_REAL)
#undef X

// Householder QR (lib.rs:667-671 params, :1520-1559 factor, :1560-1660 solves, :1661-1720 reconstruct and inverse)
#define X(suf, T)                                                                                                      \
	FaerQrParams libfaer_v0_23_QrParams_##suf(void) { return FaerQrParams{48 * 48, 192 * 256}; }                   \
	size_t libfaer_v0_23_qr_recommended_block_size_##suf(size_t nrows, size_t ncols)                               \
	{                                                                                                              \
		return qr_block_size(nrows, ncols);                                                                    \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_factor_in_place_scratch_##suf(size_t, size_t ncols, size_t bs, FaerPar,            \
								  FaerQrParams)                                        \
	{                                                                                                              \
		return layout(bs * ncols * sizeof(T), 64);                                                             \
	}                                                                                                              \
	FaerQrStatus libfaer_v0_23_qr_factor_in_place_##suf(FaerMatMut A, FaerMatMut Q, FaerPar, FaerMemAlloc,         \
							    FaerQrParams params)                                       \
	{                                                                                                              \
		return qr_api<T>(A, Q, params);                                                                        \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_solve_in_place_scratch_##suf(size_t, size_t bs, size_t k, FaerPar)                 \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_qr_solve_in_place_##suf(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj,               \
						   FaerMatMut rhs, FaerPar, FaerMemAlloc)                              \
	{                                                                                                              \
		qr_solve_api<T>(Qb, Qc, R, rhs, false, true);                                                          \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_solve_transpose_in_place_scratch_##suf(size_t, size_t bs, size_t k, FaerPar)       \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_qr_solve_transpose_in_place_##suf(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj,     \
							     FaerMatMut rhs, FaerPar, FaerMemAlloc)                    \
	{                                                                                                              \
		qr_solve_api<T>(Qb, Qc, R, rhs, true, true);                                                           \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_solve_lstsq_in_place_scratch_##suf(size_t, size_t, size_t bs, size_t k, FaerPar)   \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_qr_solve_lstsq_in_place_##suf(FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj,         \
							 FaerMatMut rhs, FaerPar, FaerMemAlloc)                        \
	{                                                                                                              \
		qr_solve_api<T>(Qb, Qc, R, rhs, false, false);                                                         \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_reconstruct_scratch_##suf(size_t, size_t ncols, size_t bs, FaerPar)                \
	{                                                                                                              \
		return layout(bs * ncols * sizeof(T), 64);                                                             \
	}                                                                                                              \
	void libfaer_v0_23_qr_reconstruct_##suf(FaerMatMut A, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerPar,     \
						FaerMemAlloc)                                                          \
	{                                                                                                              \
		qr_reconstruct_api<T>(A, Qb, Qc, R);                                                                   \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_qr_inverse_scratch_##suf(size_t dim, size_t bs, FaerPar)                              \
	{                                                                                                              \
		return layout(bs * dim * sizeof(T), 64);                                                               \
	}                                                                                                              \
	void libfaer_v0_23_qr_inverse_##suf(FaerMatMut A_inv, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerPar,     \
					    FaerMemAlloc)                                                              \
	{                                                                                                              \
		qr_inverse_api<T>(A_inv, Qb, Qc, R);                                                                   \
	}
FH_FOR_REAL(X)
#undef X

// Householder application (lib.rs:1423-1470 on the left, :1471-1518 on the right)
#define X(suf, T)                                                                                                      \
	FaerLayout libfaer_v0_23_apply_householder_on_the_left_scratch_##suf(size_t, size_t bs, size_t k)              \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_apply_householder_on_the_left_##suf(FaerMatRef V, FaerMatRef H, FaerConj, FaerMatMut rhs,   \
							       FaerPar, FaerMemAlloc)                                  \
	{                                                                                                              \
		apply_hh_api<T>(V, H, rhs, false);                                                                     \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_left_scratch_##suf(size_t, size_t bs, size_t k)    \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_apply_householder_transpose_on_the_left_##suf(FaerMatRef V, FaerMatRef H, FaerConj,         \
									 FaerMatMut rhs, FaerPar, FaerMemAlloc)        \
	{                                                                                                              \
		apply_hh_api<T>(V, H, rhs, true);                                                                      \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_apply_householder_on_the_right_scratch_##suf(size_t, size_t bs, size_t k)             \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_apply_householder_on_the_right_##suf(FaerMatRef V, FaerMatRef H, FaerConj, FaerMatMut M,    \
								FaerPar, FaerMemAlloc)                                 \
	{                                                                                                              \
		apply_hh_right_api<T>(V, H, M, false);                                                                 \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_apply_householder_transpose_on_the_right_scratch_##suf(size_t, size_t bs, size_t k)   \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_apply_householder_transpose_on_the_right_##suf(FaerMatRef V, FaerMatRef H, FaerConj,        \
									  FaerMatMut M, FaerPar, FaerMemAlloc)         \
	{                                                                                                              \
		apply_hh_right_api<T>(V, H, M, true);                                                                  \
	}
FH_FOR_REAL(X)
#undef X

// column-pivot QR (lib.rs:1721-1876 factor and solves, :1877-1950 reconstruct and inverse)
#define X(suf, T)                                                                                                      \
	FaerColPivQrParams libfaer_v0_23_ColPivQrParams_##suf(void) { return FaerColPivQrParams{48 * 48, 192 * 256}; }
FH_FOR_REAL(X)
#undef X
#define X(suf, T, it, I)                                                                                               \
	FaerLayout libfaer_v0_23_colpiv_qr_factor_in_place_scratch_##it##_##suf(size_t, size_t ncols, size_t, FaerPar, \
										 FaerColPivQrParams)                   \
	{                                                                                                              \
		return layout(ncols * 2 * sizeof(T), 64);                                                              \
	}                                                                                                              \
	FaerColPivQrStatus libfaer_v0_23_colpiv_qr_factor_in_place_##it##_##suf(                                       \
		FaerMatMut A, FaerMatMut Q_coeff, FaerSliceMut pf, FaerSliceMut pb, FaerPar, FaerMemAlloc,             \
		FaerColPivQrParams)                                                                                    \
	{                                                                                                              \
		return colpiv_qr_api<T, I>(A, Q_coeff, pf, pb);                                                        \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_colpiv_qr_solve_in_place_scratch_##it##_##suf(size_t, size_t bs, size_t k, FaerPar)   \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_colpiv_qr_solve_in_place_##it##_##suf(                                                      \
		FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj, FaerSliceRef pf, FaerSliceRef pb,                \
		FaerMatMut rhs, FaerPar, FaerMemAlloc)                                                                 \
	{                                                                                                              \
		colpiv_qr_solve_api<T, I>(Qb, Qc, R, pf, pb, rhs, false, true);                                        \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_colpiv_qr_solve_transpose_in_place_scratch_##it##_##suf(size_t, size_t bs, size_t k,  \
											  FaerPar)                     \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_colpiv_qr_solve_transpose_in_place_##it##_##suf(                                            \
		FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj, FaerSliceRef pf, FaerSliceRef pb,                \
		FaerMatMut rhs, FaerPar, FaerMemAlloc)                                                                 \
	{                                                                                                              \
		colpiv_qr_solve_api<T, I>(Qb, Qc, R, pf, pb, rhs, true, true);                                         \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_scratch_##it##_##suf(size_t, size_t, size_t bs,        \
										      size_t k, FaerPar)               \
	{                                                                                                              \
		return layout(bs * k * sizeof(T), 64);                                                                 \
	}                                                                                                              \
	void libfaer_v0_23_colpiv_qr_solve_lstsq_in_place_##it##_##suf(                                                \
		FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerConj, FaerSliceRef pf, FaerSliceRef pb,                \
		FaerMatMut rhs, FaerPar, FaerMemAlloc)                                                                 \
	{                                                                                                              \
		colpiv_qr_solve_api<T, I>(Qb, Qc, R, pf, pb, rhs, false, false);                                       \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_colpiv_qr_reconstruct_scratch_##it##_##suf(size_t, size_t ncols, size_t bs, FaerPar)  \
	{                                                                                                              \
		return layout(bs * ncols * sizeof(T), 64);                                                             \
	}                                                                                                              \
	void libfaer_v0_23_colpiv_qr_reconstruct_##it##_##suf(                                                         \
		FaerMatMut A, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerSliceRef pf, FaerSliceRef pb, FaerPar,   \
		FaerMemAlloc)                                                                                          \
	{                                                                                                              \
		colpiv_qr_reconstruct_api<T, I>(A, Qb, Qc, R, pf, pb);                                                 \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_colpiv_qr_inverse_scratch_##it##_##suf(size_t dim, size_t bs, FaerPar)                \
	{                                                                                                              \
		return layout(bs * dim * sizeof(T), 64);                                                               \
	}                                                                                                              \
	void libfaer_v0_23_colpiv_qr_inverse_##it##_##suf(                                                             \
		FaerMatMut A_inv, FaerMatRef Qb, FaerMatRef Qc, FaerMatRef R, FaerSliceRef pf, FaerSliceRef pb,        \
		FaerPar, FaerMemAlloc)                                                                                 \
	{                                                                                                              \
		colpiv_qr_inverse_api<T, I>(A_inv, Qb, Qc, R, pf, pb);                                                 \
	}
FH_FOR_INDEXED(FH_FOR_REAL)
#undef X

FaerPar libfaer_v0_23_get_global_par(void)
{
	FaerPar p;
	p.tag = (FaerParTag) g_par_tag.load();
	p.nthreads = p.tag == FaerParTag_Seq ? 1 : g_par_threads.load();
	return p;
}
void libfaer_v0_23_set_global_par(FaerPar par)
{
	g_par_tag.store((int) par.tag);
	g_par_threads.store(par.nthreads);
}

// ---------------------------------------------------------------------------------------- runtime control
const char *faer_hip_version(void) { return "faer_hip 0.1 gfx950"; }

int faer_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		(void) hipGetLastError();
		return 0;
	}
	int ok = 0;
	for (int d = 0; d < n; ++d) {
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
			++ok;
	}
	return ok;
}
void faer_hip_set_device(int device)
{
	FH_HIP(hipSetDevice(device));
	Ctx &c = ctx();
	c.device = device;
}
void faer_hip_set_stream(void *s) { ctx().set_stream(static_cast<hipStream_t>(s)); }
void *faer_hip_get_stream(void) { return ctx().stream; }
void faer_hip_synchronize(void) { ctx().sync(); }
void faer_hip_shutdown(void) { fh::ctx_shutdown(); }
void *faer_hip_malloc(size_t bytes)
{
	ctx();
	void *p = nullptr;
	FH_HIP(hipMalloc(&p, bytes ? bytes : 1));
	return p;
}
void faer_hip_free(void *p)
{
	if (p)
		FH_HIP(hipFree(p));
}
void faer_hip_memcpy_h2d(void *d, const void *s, size_t bytes)
{
	FH_HIP(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, ctx().stream));
	ctx().sync();
}
void faer_hip_memcpy_d2h(void *d, const void *s, size_t bytes)
{
	FH_HIP(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, ctx().stream));
	ctx().sync();
}
void faer_hip_set_gemm_variant(int v) { ctx().gemm_variant = v; }
void faer_hip_debug_stream_xcc(int which, int nblocks, unsigned *out_host) { debug_stream_xcc(which, nblocks, out_host); }
size_t faer_hip_debug_llt_plan(size_t n, size_t tail_rows, size_t nb2, size_t *starts, size_t cap)
{
	const std::vector<idx_t> J = llt_plan((idx_t) n, (idx_t) tail_rows, (idx_t) nb2);
	for (size_t i = 0; i < J.size() && i < cap; ++i)
		starts[i] = (size_t) J[i];
	return J.size();
}
size_t faer_hip_debug_llt_steps(size_t n, size_t la_min, size_t tail_rows, size_t side_rmin, size_t dpanel_rmin, int *codes, size_t cap)
{
	return llt_debug_steps((idx_t) n, (idx_t) la_min, (idx_t) tail_rows, (idx_t) side_rmin, (idx_t) dpanel_rmin, codes, cap);
}
int faer_hip_debug_gemm_plan(const long long q[24], int out[16], const char **refusal)
{
	if (refusal)
		*refusal = nullptr;
	for (int i = 0; i < 3; ++i)
		if (q[i] < 1 || q[i] >= (1LL << 31))
			return -1;
	if ((q[3] != 4 && q[3] != 8) || q[4] < 0 || q[4] > 2 || q[15] < 0 || q[15] > 6 || q[16] < 0 || q[16] > 6 || q[17] < 0 || q[17] > 2)
		return -1;
	GemmProblem p{(idx_t) q[0], (idx_t) q[1], (idx_t) q[2], (int) q[3], (DstKind) q[4], q[5] != 0, (int) q[6], (idx_t) q[7], (idx_t) q[8],
		      (idx_t) q[9], (idx_t) q[10], (idx_t) q[11], (idx_t) q[12], q[13] != 0, q[14] != 0, (int) q[15], (int) q[16], (int) q[17],
		      (idx_t) q[18], (idx_t) q[19], (idx_t) q[20], (idx_t) q[21], q[22] != 0, (int) q[23], false};
	gemm_orient(p);
	GemmPlan g;
	const char *why = gemm_plan(p, g);
	if (why) {
		if (refusal)
			*refusal = why;
		return 1;
	}
	const int v[16] = {g.transposed, (int) g.tile, g.tri_skip_split, g.akm, g.bkm, g.bm, g.bn, g.ntm, g.ntn, g.tri_enum, g.tri_off, g.splits,
			   g.k_per_split, g.fast_io, g.prof_class, (int) g.routes};
	memcpy(out, v, sizeof(v));
	return 0;
}
void faer_hip_debug_dump_timing(void)
{
	trsm_dump_timing();
	lu_dump_timing();
	gemm_dump_timing();
}

#define X(suf, T)                                                                                                      \
	FaerTridiagParams libfaer_v0_23_TridiagParams_##suf(void) { return FaerTridiagParams{192 * 256}; }              \
	FaerSelfAdjointEvdParams libfaer_v0_23_SelfAdjointEvdParams_##suf(void)                                        \
	{                                                                                                              \
		return FaerSelfAdjointEvdParams{FaerTridiagParams{192 * 256}, 128};                                    \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_self_adjoint_evd_scratch_##suf(size_t dim, FaerComputeEigenvectors compute_U, FaerPar par, \
								  FaerSelfAdjointEvdParams params)                          \
	{                                                                                                              \
		(void) compute_U;                                                                                      \
		(void) par;                                                                                            \
		(void) params;                                                                                         \
		return layout((2 * dim * dim + 12 * dim) * sizeof(T), 64);                                             \
	}                                                                                                              \
	FaerEvdStatus libfaer_v0_23_self_adjoint_evd_##suf(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerPar par,      \
							   FaerMemAlloc mem, FaerSelfAdjointEvdParams params)               \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) mem;                                                                                            \
		return self_adjoint_evd_api<T>(A, U, S, params);                                                       \
	}
FH_FOR_DTYPES(X)
#undef X

#define X(suf, T)                                                                                                      \
	FaerBidiagParams libfaer_v0_23_BidiagParams_##suf(void) { return FaerBidiagParams{192 * 256}; }                 \
	FaerSvdParams libfaer_v0_23_SvdParams_##suf(void)                                                              \
	{                                                                                                              \
		return FaerSvdParams{FaerBidiagParams{192 * 256}, libfaer_v0_23_QrParams_##suf(), 128, 11.0 / 6.0};     \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_svd_scratch_##suf(size_t nrows, size_t ncols, FaerComputeSvdVectors compute_U,        \
						   FaerComputeSvdVectors compute_V, FaerPar par, FaerSvdParams params)  \
	{                                                                                                              \
		(void) compute_U;                                                                                      \
		(void) compute_V;                                                                                      \
		(void) par;                                                                                            \
		(void) params;                                                                                         \
		const size_t big = nrows < ncols ? ncols : nrows, small = nrows < ncols ? nrows : ncols;               \
		if (small == 0)                                                                                        \
			return layout(0, 1); /* StackReq::EMPTY (mod.rs:483-485) */                                    \
		return layout((2 * big * small + 8 * (small + 1) * (small + 1) + 64 * (small + 1)) * sizeof(T), 64);   \
	}                                                                                                              \
	FaerSvdStatus libfaer_v0_23_svd_##suf(FaerMatRef A, FaerMatMut U, FaerVecMut S, FaerMatMut V, FaerPar par,     \
					      FaerMemAlloc mem, FaerSvdParams params)                                   \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) mem;                                                                                            \
		return svd_api<T>(A, U, S, V, params);                                                                 \
	}
FH_FOR_DTYPES(X)
#undef X

size_t faer_hip_default_recommended_shift_count(size_t n, size_t active)
{
	(void) active; // evd/schur/mod.rs:59-79
	return n < 30 ? 2 : n < 60 ? 4 : n < 150 ? 12 : n < 590 ? 32 : n < 3000 ? 64 : n < 6000 ? 128 : 256;
}
size_t faer_hip_default_recommended_deflation_window(size_t n, size_t active)
{
	(void) active; // evd/schur/mod.rs:80-107
	if (n < 30)
		return 2;
	if (n < 60)
		return 4;
	if (n < 150)
		return 10;
	if (n < 590)
		return (size_t) ((double) n / log2((double) n));
	return n < 3000 ? 96 : n < 6000 ? 192 : 384;
}
void faer_hip_debug_evd_last_counts(long out[4]) { evd_last_counts(out); }
size_t faer_hip_evd_window_edge(FaerHipDType dtype) { return (size_t) schur_window_edge(dtype == FaerHipDType_F64 ? 8 : 4); }

#define X(suf, T)                                                                                                      \
	FaerHessenbergParams libfaer_v0_23_HessenbergParams_##suf(void) { return FaerHessenbergParams{192 * 256, 256 * 256}; } \
	FaerSchurParams libfaer_v0_23_SchurParams_##suf(void)                                                          \
	{                                                                                                              \
		return FaerSchurParams{faer_hip_default_recommended_shift_count, faer_hip_default_recommended_deflation_window, 75, 50}; \
	}                                                                                                              \
	FaerEvdFromSchurParams libfaer_v0_23_EvdFromSchurParams_##suf(void) { return FaerEvdFromSchurParams{64}; }      \
	FaerEvdParams libfaer_v0_23_EvdParams_##suf(void)                                                              \
	{                                                                                                              \
		return FaerEvdParams{libfaer_v0_23_HessenbergParams_##suf(), libfaer_v0_23_SchurParams_##suf(),        \
				     libfaer_v0_23_EvdFromSchurParams_##suf()};                                        \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_evd_scratch_##suf(size_t dim, FaerComputeEigenvectors compute_left,                   \
						   FaerComputeEigenvectors compute_right, FaerPar par, FaerEvdParams params) \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) params;                                                                                         \
		if (dim == 0)                                                                                          \
			return layout(0, 1); /* StackReq::EMPTY (mod.rs:968-970) */                                    \
		/* the reference asks for H, Z and the largest of {householder + reduction, the sweep's workspace, X} */ \
		const bool vec = compute_left == FaerComputeEigenvectors_Yes || compute_right == FaerComputeEigenvectors_Yes; \
		return layout(evd_arena_bytes((idx_t) dim, vec, (idx_t) qr_block_size(dim - 1, dim - 1) + 1, (int) sizeof(T)) + 3 * dim * dim * sizeof(T), 64); \
	}                                                                                                              \
	FaerEvdStatus libfaer_v0_23_evd_##suf(FaerMatRef A, FaerMatMut UL, FaerMatMut UR, FaerVecMut S, FaerVecMut S_im, \
					      FaerPar par, FaerMemAlloc mem, FaerEvdParams params)                      \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) mem;                                                                                            \
		return evd_api<T>(A, UL, UR, S, S_im, params);                                                         \
	}
FH_FOR_DTYPES(X)
#undef X

size_t faer_hip_default_relative_cost_estimate_of_shift_chase_to_matmul(size_t n, size_t active)
{
	(void) n;
	(void) active; // gevd/mod.rs:85-91
	return 10;
}
void faer_hip_debug_gevd_last_counts(long out[5]) { gevd_last_counts(out); }
size_t faer_hip_gevd_window_edge(FaerHipDType dtype) { return (size_t) gevd_window_edge(dtype == FaerHipDType_F64 ? 8 : 4); }

#define X(suf, T)                                                                                                      \
	FaerGeneralizedHessenbergParams libfaer_v0_23_GeneralizedHessenbergParams_##suf(void)                          \
	{                                                                                                              \
		return FaerGeneralizedHessenbergParams{32, 256 * 256}; /* gen_hessenberg/mod.rs */                     \
	}                                                                                                              \
	FaerGeneralizedSchurParams libfaer_v0_23_GeneralizedSchurParams_##suf(void)                                    \
	{                                                                                                              \
		const FaerSchurParams sp = libfaer_v0_23_SchurParams_##suf(); /* gevd/mod.rs:92-105 */                  \
		return FaerGeneralizedSchurParams{faer_hip_default_relative_cost_estimate_of_shift_chase_to_matmul, sp.recommended_shift_count, \
						  sp.recommended_deflation_window, sp.blocking_threshold, sp.nibble_threshold}; \
	}                                                                                                              \
	FaerGevdParams libfaer_v0_23_GevdParams_##suf(void)                                                            \
	{                                                                                                              \
		return FaerGevdParams{libfaer_v0_23_GeneralizedHessenbergParams_##suf(), libfaer_v0_23_GeneralizedSchurParams_##suf(), \
				      FaerGevdFromSchurParams{0}};                                                      \
	}                                                                                                              \
	FaerLayout libfaer_v0_23_generalized_evd_scratch_##suf(size_t dim, FaerComputeEigenvectors compute_left,      \
							       FaerComputeEigenvectors compute_right, FaerPar par, FaerGevdParams params) \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) params;                                                                                         \
		if (dim == 0)                                                                                          \
			return layout(0, 1);                                                                           \
		const bool vec = compute_left == FaerComputeEigenvectors_Yes || compute_right == FaerComputeEigenvectors_Yes; \
		/* the arena of the call with every operand staged */                                                  \
		return layout(gevd_arena_bytes((idx_t) dim, vec, (idx_t) qr_block_size(dim, dim) + 1, (int) sizeof(T)) + 4 * dim * dim * sizeof(T) \
				      + 3 * dim * sizeof(T), 64);                                                       \
	}                                                                                                              \
	FaerGevdStatus libfaer_v0_23_generalized_evd_##suf(FaerMatMut A, FaerMatMut B, FaerMatMut UL, FaerMatMut UR, FaerVecMut alpha, \
							   FaerVecMut alpha_im, FaerVecMut beta, FaerPar par, FaerMemAlloc mem, \
							   FaerGevdParams params)                                       \
	{                                                                                                              \
		(void) par;                                                                                            \
		(void) mem;                                                                                            \
		return gevd_api<T>(A, B, UL, UR, alpha, alpha_im, beta, params);                                       \
	}
FH_FOR_DTYPES(X)
#undef X

void faer_hip_tridiag_in_place_f64(FaerMatMut A, FaerMatMut householder) { tridiag_api<double>(A, householder); }
void faer_hip_tridiag_in_place_f32(FaerMatMut A, FaerMatMut householder) { tridiag_api<float>(A, householder); }
void faer_hip_bidiag_in_place_f64(FaerMatMut A, FaerMatMut Hl, FaerMatMut Hr) { bidiag_api<double>(A, Hl, Hr); }
void faer_hip_bidiag_in_place_f32(FaerMatMut A, FaerMatMut Hl, FaerMatMut Hr) { bidiag_api<float>(A, Hl, Hr); }
void faer_hip_hessenberg_in_place_f64(FaerMatMut A, FaerMatMut householder) { hessenberg_api<double>(A, householder); }
void faer_hip_hessenberg_in_place_f32(FaerMatMut A, FaerMatMut householder) { hessenberg_api<float>(A, householder); }

// Cholesky update and deletion (cholesky/llt/update.rs:360-379, cholesky/ldlt/update.rs:376-434; no faer-ffi entry points)
#define X(suf, T)                                                                                                      \
	FaerLltStatus faer_hip_llt_rank_r_update_clobber_##suf(FaerMatMut L, FaerMatMut W, FaerVecMut alpha)           \
	{                                                                                                              \
		return chol_update_api<T>(L, W, alpha, false);                                                         \
	}                                                                                                              \
	void faer_hip_ldlt_rank_r_update_clobber_##suf(FaerMatMut LD, FaerMatMut W, FaerVecMut alpha)                  \
	{                                                                                                              \
		(void) chol_update_api<T>(LD, W, alpha, true);                                                         \
	}                                                                                                              \
	FaerLayout faer_hip_ldlt_delete_rows_and_cols_clobber_scratch_##suf(size_t dim, size_t n_removed)              \
	{                                                                                                              \
		return layout((dim * n_removed + n_removed) * sizeof(T), 64); /* ldlt/update.rs:402-408 */             \
	}
FH_FOR_DTYPES(X)
#undef X
#define X(suf, T, it, I)                                                                                               \
	void faer_hip_ldlt_delete_rows_and_cols_clobber_##it##_##suf(FaerMatMut LD, FaerSliceMut indices, FaerPar,     \
								     FaerMemAlloc)                                     \
	{                                                                                                              \
		ldlt_delete_api<T, I>(LD, indices);                                                                    \
	}
FH_FOR_INDEXED(FH_FOR_DTYPES)
#undef X
void faer_hip_debug_chol_update_last(long out[4]) { chol_update_last(out); }
void faer_hip_debug_chol_update_diag_only(int on) { chol_update_debug_diag_only(on); }
void faer_hip_chol_update_shape(int dtype, size_t out[2]) { chol_update_shape(dtype == (int) FaerHipDType_F64 ? 8 : 4, out); }
void faer_hip_debug_clu_shape(int dtype, size_t out[2]) { clu_shape(dtype == (int) FaerHipDType_C64 ? 16 : 8, out); }
void faer_hip_debug_clu_last(size_t out[4]) { clu_last(out); }

int faer_hip_debug_lu_leaf_width(size_t nrows, FaerHipDType dtype, int resident_workgroups)
{
	return lu_leaf_width((idx_t) nrows, dtype == FaerHipDType_F64 ? 8 : 4, resident_workgroups);
}
int faer_hip_debug_dist_two_streams_ok(size_t panel_rows, FaerHipDType dtype, int panel_cus, int all_cus)
{
	return dist_two_streams_ok((idx_t) panel_rows, dtype == FaerHipDType_F64 ? 8 : 4, panel_cus, all_cus) ? 1 : 0;
}
void faer_hip_debug_lu_force_general(int on) { lu_force_general(on); }
void faer_hip_debug_lu_plan(size_t nb2_from, size_t pipe_from, size_t la_min_cols) { lu_debug_plan((long) nb2_from, (long) pipe_from, (long) la_min_cols); }
long faer_hip_debug_qr_one_pass_columns(void) { return qr_last_one_pass_columns(); }
void faer_hip_debug_route_reset(void)
{
	for (long long &c : g_route_counts)
		c = 0;
}
size_t faer_hip_debug_route_counts(long long *out, size_t cap)
{
	for (size_t i = 0; i < cap && i < (size_t) FaerHipRoute_Count; ++i)
		out[i] = g_route_counts[i];
	return (size_t) FaerHipRoute_Count;
}
void faer_hip_debug_qr_panel_copy(int on) { tsqr_debug_panel_copy(on); }
void faer_hip_debug_qr_one_pass_f64(int on) { tsqr_debug_f64(on); }
void faer_hip_debug_qr_panels_one_pass(int on) { tsqr_debug_panels(on); }
void faer_hip_debug_qr_one_pass_shape_rule(long min_rows, long min_rows_per_column) { tsqr_debug_shape_rule(min_rows, min_rows_per_column); }
void faer_hip_debug_fplu_inplace(int on) { fplu_debug_inplace(on); }
void faer_hip_debug_level2_force_memory_bodies(int on) { level2_debug_force_memory_bodies(on); }
void faer_hip_debug_scratch_fill(int byte_or_minus_one) { debug_scratch_fill(byte_or_minus_one); }
void faer_hip_debug_scratch_fill_stats(size_t out[2]) { debug_scratch_fill_stats(out); }
void *faer_hip_debug_internal_stream(int which)
{
	Ctx &c = ctx();
	FH_CHECK(c.lookahead_streams(), "debug_internal_stream: look-ahead streams unavailable");
	return which == 1 ? (void *) c.la_bulk : (void *) c.la_panel;
}

double faer_hip_time_gemm_ms(FaerHipDType dtype, size_t m, size_t n, size_t k, void *dst, ptrdiff_t dst_cs, const void *lhs,
			     ptrdiff_t lhs_cs, const void *rhs, ptrdiff_t rhs_cs, int iters)
{
	FH_CHECK(is_device_ptr(dst) && is_device_ptr(lhs) && is_device_ptr(rhs), "time_gemm: operands must be device memory");
	if (dtype == FaerHipDType_F64)
		return gemm_time_ms<double>(MatV<double>{(double *) dst, (idx_t) m, (idx_t) n, 1, (idx_t) dst_cs},
					    MatV<const double>{(const double *) lhs, (idx_t) m, (idx_t) k, 1, (idx_t) lhs_cs},
					    MatV<const double>{(const double *) rhs, (idx_t) k, (idx_t) n, 1, (idx_t) rhs_cs}, iters);
	FH_CHECK(dtype == FaerHipDType_F32, "time_gemm: f32/f64 only");
	return gemm_time_ms<float>(MatV<float>{(float *) dst, (idx_t) m, (idx_t) n, 1, (idx_t) dst_cs},
				   MatV<const float>{(const float *) lhs, (idx_t) m, (idx_t) k, 1, (idx_t) lhs_cs},
				   MatV<const float>{(const float *) rhs, (idx_t) k, (idx_t) n, 1, (idx_t) rhs_cs}, iters);
}
double faer_hip_mfma_peak_tflops(FaerHipDType dtype, int iters) { return mfma_peak_tflops(dtype == FaerHipDType_F64, iters); }

void faer_hip_prof_begin(void)
{
	Ctx &c = ctx();
	double scratch[Ctx::PROF_CLASSES * 3];
	prof_collect(scratch); // (drops spans of an unfinished profile)
	c.prof_on = true;
}
void faer_hip_prof_end(double *out18)
{
	FH_CHECK(out18 != nullptr, "prof_end: NULL output");
	Ctx &c = ctx();
	c.prof_on = false;
	FH_HIP(hipDeviceSynchronize());
	prof_collect(out18);
}
size_t faer_hip_prof_end_spans(double *out18, double *spans, size_t cap)
{
	FH_CHECK(out18 != nullptr && (spans != nullptr || cap == 0), "prof_end_spans: NULL output");
	Ctx &c = ctx();
	c.prof_on = false;
	FH_HIP(hipDeviceSynchronize());
	size_t n = 0;
	prof_collect(out18, spans, cap, &n);
	return n;
}
double faer_hip_xwg_hop_us(int iters) { return xwg_hop_us(iters); }
void faer_hip_partial_piv_lu_lend_copy(const void *device_copy, size_t nrows, size_t ncols, int elem_bytes)
{
	lu_lend_copy(device_copy, (idx_t) nrows, (idx_t) ncols, elem_bytes);
}

} // extern "C"
