// Helpers shared by the symmetric factorizations with a permutation (lblt.hip, piv_llt.hip): boundary views, the upload of a host
// permutation, the row gather X <- X[perm, :] and the permuted symmetric write-back into a lower triangle.
#pragma once
#include "common.h"

namespace fh {

// lower(out)[i, j] = tmp[max(p_i, p_j), min(p_i, p_j)], p = perm_inv (reconstruct.rs:72-83); tmp n x n column major
template <typename T> __global__ void lblt_sym_gather_kernel(T *out, idx_t rs, idx_t cs, idx_t n, const T *tmp, const idx_t *pinv)
{
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
	if (i >= n || j > i)
		return;
	const idx_t pi = pinv[i], pj = pinv[j];
	out[i * rs + j * cs] = pi >= pj ? tmp[pi + pj * n] : tmp[pj + pi * n];
}

namespace {

template <typename T> MatV<const T> view(FaerMatRef m)
{
	return MatV<const T>{static_cast<const T *>(m.ptr), (idx_t) m.nrows, (idx_t) m.ncols, (idx_t) m.row_stride, (idx_t) m.col_stride};
}
template <typename T> MatV<T> view(FaerMatMut m)
{
	return MatV<T>{static_cast<T *>(m.ptr), (idx_t) m.nrows, (idx_t) m.ncols, (idx_t) m.row_stride, (idx_t) m.col_stride};
}
template <typename T> MatV<const T> vview(FaerVecRef v) { return MatV<const T>{static_cast<const T *>(v.ptr), (idx_t) v.len, 1, (idx_t) v.stride, 0}; }
template <typename T> MatV<T> vview(FaerVecMut v) { return MatV<T>{static_cast<T *>(v.ptr), (idx_t) v.len, 1, (idx_t) v.stride, 0}; }

template <typename I> void upload_perm(Scratch &buf, const void *perm_host, idx_t n)
{
	std::vector<idx_t> p64((size_t) n);
	for (idx_t i = 0; i < n; ++i) {
		p64[(size_t) i] = (idx_t) static_cast<const I *>(perm_host)[i];
		FH_CHECK(p64[(size_t) i] >= 0 && p64[(size_t) i] < n, "permutation index out of range");
	}
	FH_HIP(hipMemcpyAsync(buf.p, p64.data(), (size_t) n * sizeof(idx_t), hipMemcpyHostToDevice, ctx().stream));
	ctx().sync(); // p64 goes out of scope
}

// X[i, :] <- X[perm[i], :]
template <typename T, typename I> void permute_rows(MatV<T> X, const void *perm_host)
{
	const idx_t n = X.nrows, k = X.ncols;
	Scratch pb((size_t) n * sizeof(idx_t)), tb((size_t) n * (size_t) k * sizeof(T));
	upload_perm<I>(pb, perm_host, n);
	MatV<T> tmp{tb.as<T>(), n, k, 1, n};
	gather_rows_dev<T>(tmp, X.c(), pb.as<idx_t>());
	copy_dev<T>(X, tmp.c());
	ctx().sync();
}

} // namespace
} // namespace fh
