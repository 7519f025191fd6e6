// The one permutation and boundary-view layer of the solve / reconstruct / inverse side (api.hip, lblt.hip, piv_llt.hip) and of the
// factor drivers that turn pivot records into permutations (getrf.hip, fplu.hip, lblt.hip, piv_llt.hip, colpiv_qr.hip):
//   * host only: perm_from_transpositions / invert_perm -- permutation, inverse and transposition count from pivot records;
//   * boundary: view / vview / layout, store_perm (a factorization's permutations into the caller's u32 / u64 slices);
//   * device: DevPerm (a caller's permutation slice, validated and uploaded once), permute_rows, gather_rows_cols, sym_gather.
// FH_PERM_HOST_ONLY leaves the host-only part alone, without any HIP header (the stand-alone program of tests/test_perm_host.py).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <utility>

#ifndef FH_PERM_HOST_ONLY
#include "common.h"
#endif

namespace fh {

#ifdef FH_PERM_HOST_ONLY
typedef long idx_t;
#endif

// every check of this layer fails the same way: "faer_hip: fatal: <who>: <what>"
[[noreturn]] inline void perm_die(const char *who, const char *what)
{
	fprintf(stderr, "faer_hip: fatal: %s: %s\n", who, what);
	fflush(stderr);
	abort();
}

inline void invert_perm(idx_t n, const idx_t *perm, idx_t *perm_inv)
{
	for (idx_t i = 0; i < n; ++i)
		perm_inv[perm[i]] = i;
}

// perm = the identity of n entries with the transpositions (j <-> record(j)), j = 0 .. nrecords - 1, applied in order; perm_inv
// its inverse; returns how many of them moved something.  A record names a row at or below its own: j <= record(j) < n;
// record is called once per j, in ascending order (lblt.hip walks its block starts along with it).
template <typename Record> long perm_from_transpositions(const char *who, idx_t n, idx_t nrecords, Record record, idx_t *perm, idx_t *perm_inv)
{
	for (idx_t i = 0; i < n; ++i)
		perm[i] = i;
	long count = 0;
	for (idx_t j = 0; j < nrecords; ++j) {
		const idx_t p = record(j);
		if (p < j || p >= n)
			perm_die(who, "pivot record out of range");
		if (p != j) {
			std::swap(perm[j], perm[p]);
			++count;
		}
	}
	invert_perm(n, perm, perm_inv);
	return count;
}

#ifndef FH_PERM_HOST_ONLY

// ---- boundary views
template <typename T> MatV<const T> view(FaerMatRef m)
{
	return MatV<const T>{static_cast<const T *>(m.ptr), (idx_t) m.nrows, (idx_t) m.ncols, (idx_t) m.row_stride, (idx_t) m.col_stride};
}
template <typename T> MatV<T> view(FaerMatMut m)
{
	return MatV<T>{static_cast<T *>(m.ptr), (idx_t) m.nrows, (idx_t) m.ncols, (idx_t) m.row_stride, (idx_t) m.col_stride};
}
// a vector as an n x 1 view (stride in elements)
template <typename T> MatV<const T> vview(FaerVecRef v) { return MatV<const T>{static_cast<const T *>(v.ptr), (idx_t) v.len, 1, (idx_t) v.stride, 0}; }
template <typename T> MatV<T> vview(FaerVecMut v) { return MatV<T>{static_cast<T *>(v.ptr), (idx_t) v.len, 1, (idx_t) v.stride, 0}; }

inline FaerLayout layout(size_t bytes, size_t align) { return FaerLayout{bytes, align}; }

// ---- permutation slices of the boundary: host memory, u32 or u64 entries
// a slice an entry point reads (at least n entries) or writes (exactly n)
inline void check_perm_slice(const char *who, const void *ptr, size_t len, idx_t n, bool exact)
{
	if (exact ? (idx_t) len != n : (idx_t) len < n)
		perm_die(who, exact ? "a permutation slice does not have exactly one entry per row / column" : "a permutation slice is too short");
	if (is_device_ptr(ptr))
		perm_die(who, "permutation slices must be host memory");
}

inline void check_perm_slice(const char *who, FaerSliceRef s, idx_t n) { check_perm_slice(who, s.ptr, s.len, n, false); }

// what a factor entry point does with the permutations its driver returned
template <typename I> void store_perm(const char *who, FaerSliceMut fwd, FaerSliceMut bwd, const idx_t *perm, const idx_t *perm_inv, idx_t n)
{
	check_perm_slice(who, fwd.ptr, fwd.len, n, true);
	check_perm_slice(who, bwd.ptr, bwd.len, n, true);
	I *f = static_cast<I *>(fwd.ptr), *b = static_cast<I *>(bwd.ptr);
	for (idx_t i = 0; i < n; ++i) {
		f[i] = (I) perm[i];
		b[i] = (I) perm_inv[i];
	}
}

// The first n entries of a caller's permutation slice on the device, as idx_t.  The constructor checks the slice (length, host
// memory, every index in [0, n)), uploads it and synchronises the stream: its host staging vector is gone when it returns, so a
// DevPerm may be used and destroyed at any later point without another wait -- this is the only synchronisation of this layer.
// `I{}` selects the index type of the slice.
struct DevPerm {
	idx_t n;
	Scratch buf;

	template <typename I> DevPerm(const char *who, FaerSliceRef s, idx_t n_, I) : n(n_), buf((size_t) n_ * sizeof(idx_t))
	{
		check_perm_slice(who, s.ptr, s.len, n, false);
		if (n == 0)
			return;
		std::vector<idx_t> p64((size_t) n);
		for (idx_t i = 0; i < n; ++i) {
			p64[(size_t) i] = (idx_t) static_cast<const I *>(s.ptr)[i];
			if (p64[(size_t) i] < 0 || p64[(size_t) i] >= n)
				perm_die(who, "permutation index out of range");
		}
		FH_HIP(hipMemcpyAsync(buf.p, p64.data(), (size_t) n * sizeof(idx_t), hipMemcpyHostToDevice, ctx().stream));
		ctx().sync();
	}
	const idx_t *dev() const { return buf.as<idx_t>(); }
};

// X[i, :] <- X[perm[i], :]   (perm/mod.rs:256-294 permute_rows with dst == a copy of src)
template <typename T> void permute_rows(MatV<T> X, const DevPerm &perm)
{
	const idx_t n = X.nrows, k = X.ncols;
	FH_CHECK(perm.n == n, "permute_rows: the permutation does not have one entry per row");
	if (n == 0 || k == 0)
		return;
	Scratch tb((size_t) n * (size_t) k * sizeof(T));
	MatV<T> tmp{tb.as<T>(), n, k, 1, n};
	gather_rows_dev<T>(tmp, X.c(), perm.dev());
	copy_dev<T>(X, tmp.c());
}

// out(i, j) = tmp(rows[i], cols[j])   (two gathers through a second temporary)
template <typename T> void gather_rows_cols(MatV<T> out, MatV<T> tmp, const DevPerm &rows, const DevPerm &cols)
{
	const idx_t m = out.nrows, n = out.ncols;
	FH_CHECK(rows.n == m && cols.n == n, "gather_rows_cols: the permutations do not match the matrix");
	Scratch t2((size_t) m * (size_t) n * sizeof(T) + 256);
	MatV<T> tmp2{t2.as<T>(), m, n, 1, m};
	gather_rows_dev<T>(tmp2, tmp.c(), rows.dev());
	gather_rows_dev<T>(out.t(), tmp2.t().c(), cols.dev());
}

// lower(out)[i, j] = tmp[max(p_i, p_j), min(p_i, p_j)], p = perm_inv (bunch_kaufman/reconstruct.rs:72-83, llt_pivoting/reconstruct.rs:40-51);
// tmp n x n column major, its lower triangle read
template <typename T> __global__ void sym_gather_kernel(T *out, idx_t rs, idx_t cs, idx_t n, const T *tmp, const idx_t *pinv)
{
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
	if (i >= n || j > i)
		return;
	const idx_t pi = pinv[i], pj = pinv[j];
	out[i * rs + j * cs] = pi >= pj ? tmp[pi + pj * n] : tmp[pj + pi * n];
}
template <typename T> void sym_gather(MatV<T> out, const T *tmp, const DevPerm &perm_inv)
{
	const idx_t n = out.nrows;
	FH_CHECK(perm_inv.n == n && out.ncols == n && n < 65536, "sym_gather: the permutation does not match the matrix, or the matrix is too large");
	if (n == 0)
		return;
	hipLaunchKernelGGL(sym_gather_kernel<T>, dim3((unsigned) ((n + 255) / 256), (unsigned) n), dim3(256), 0, ctx().stream, out.p, out.rs, out.cs, n,
			   tmp, perm_inv.dev());
	FH_HIP(hipGetLastError());
}

#endif // FH_PERM_HOST_ONLY

} // namespace fh
