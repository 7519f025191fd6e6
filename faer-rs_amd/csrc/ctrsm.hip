// Complex triangular solves X <- op(T)^-1 X, op = identity or conjugate, for c32 / c64.
// Blocked substitution: the matrix is halved recursively down to diagonal blocks of at most LEAF rows; a diagonal block is solved
// by plain forward substitution (never by a product with an inverted block: tests/test_stability_oracle.py says why), every
// off-diagonal update X2 -= op(L21) X1 is one launch of the complex GEMM (cgemm.hip).  An upper solve is the lower solve of the
// row- and column-reversed views.  No workspace.
#include "common.h"

namespace fh {

namespace {

constexpr int LEAF = 32;

// One thread per right-hand side.  The diagonal block (conjugated if asked) and the 64 columns of X the workgroup owns live in LDS
// as re / im planes: T is read as broadcasts, X with consecutive lanes on consecutive words.  (A register-resident column, fully
// unrolled, spills: 2 x LEAF values per lane next to LEAF^2 / 2 hoisted LDS loads.)  The strictly upper part of T -- and, unit: its
// diagonal -- is never read.  A zero pivot gives 0 / 0: the row and every row that depends on it become non-finite, the rows
// before it stay as they are.
template <typename R>
__global__ __launch_bounds__(64) void ctrsm_leaf_kernel(const Cx<R> *T, idx_t trs, idx_t tcs, int nb, int unit, int conj, Cx<R> *X, idx_t xrs,
							 idx_t xcs, int nrhs)
{
	__shared__ R tre[LEAF * LEAF], tim[LEAF * LEAF]; // T(i, j) at [j * LEAF + i]
	__shared__ R xre[LEAF * 64], xim[LEAF * 64];	 // X(i, col) at [i * 64 + tid]
	const int tid = threadIdx.x;
	for (int e = tid; e < LEAF * LEAF; e += 64) {
		const int i = e % LEAF, j = e / LEAF;
		R re = i == j ? (R) 1 : (R) 0, im = (R) 0;
		if (i < nb && j < nb && (i > j || (i == j && !unit))) {
			const Cx<R> v = T[(idx_t) i * trs + (idx_t) j * tcs];
			re = v.re;
			im = conj ? -v.im : v.im;
		}
		tre[e] = re;
		tim[e] = im;
	}
	__syncthreads();
	const int col = blockIdx.x * 64 + tid;
	if (col >= nrhs)
		return; // (no barrier below: each thread touches its own column of xre / xim only)
	Cx<R> *xp = X + (idx_t) col * xcs;
	for (int i = 0; i < nb; ++i) {
		const Cx<R> v = xp[(idx_t) i * xrs];
		xre[i * 64 + tid] = v.re;
		xim[i * 64 + tid] = v.im;
	}
	for (int j = 0; j < nb; ++j) {
		R xr = xre[j * 64 + tid], xi = xim[j * 64 + tid];
		if (!unit) { // x_j / t_jj = x_j conj(t_jj) / |t_jj|^2
			const R dr = tre[j * LEAF + j], di = tim[j * LEAF + j];
			const R den = dr * dr + di * di;
			const R qr = (xr * dr + xi * di) / den, qi = (xi * dr - xr * di) / den;
			xr = qr;
			xi = qi;
		}
		Cx<R> *p = xp + (idx_t) j * xrs;
		p->re = xr;
		p->im = xi;
		for (int i = j + 1; i < nb; ++i) {
			const R lr = tre[j * LEAF + i], li = tim[j * LEAF + i];
			xre[i * 64 + tid] -= lr * xr - li * xi;
			xim[i * 64 + tid] -= lr * xi + li * xr;
		}
	}
}

template <typename R> void ctrsm_lower_rec(MatV<const Cx<R>> L, bool unit, bool conj, MatV<Cx<R>> X)
{
	const idx_t n = L.nrows, k = X.ncols;
	if (n <= LEAF) {
		hipLaunchKernelGGL(ctrsm_leaf_kernel<R>, dim3((unsigned) ((k + 63) / 64)), dim3(64), 0, ctx().stream, L.p, L.rs, L.cs, (int) n, (int) unit,
				   (int) conj, X.p, X.rs, X.cs, (int) k);
		FH_HIP(hipGetLastError());
		return;
	}
	const idx_t h = (n / 2 + LEAF - 1) / LEAF * LEAF; // LEAF <= h < n
	ctrsm_lower_rec<R>(L.sub(0, 0, h, h), unit, conj, X.sub(0, 0, h, k));
	GemmExtra<Cx<R>> ex;
	ex.conj_lhs = conj;
	gemm_dev<Cx<R>>(X.sub(h, 0, n - h, k), DST_FULL, true, L.sub(h, 0, n - h, h), X.sub(0, 0, h, k).c(), Cx<R>{(R) -1, (R) 0}, &ex);
	ctrsm_lower_rec<R>(L.sub(h, h, n - h, n - h), unit, conj, X.sub(h, 0, n - h, k));
}

} // namespace

idx_t ctrsm_leaf_rows() { return LEAF; }

template <typename R> void ctrsm_dev(MatV<const Cx<R>> T, bool upper, bool unit, bool conj, MatV<Cx<R>> X)
{
	FH_CHECK(T.nrows == T.ncols && X.nrows == T.nrows, "triangular solve: shape mismatch");
	if (T.nrows == 0 || X.ncols == 0)
		return;
	FH_CHECK(X.ncols < (1L << 30) && T.nrows < (1L << 30), "triangular solve: dimension too large");
	ctx().ensure_device();
	if (upper)
		ctrsm_lower_rec<R>(T.rev_rows().rev_cols(), unit, conj, X.rev_rows());
	else
		ctrsm_lower_rec<R>(T, unit, conj, X);
}

template void ctrsm_dev<float>(MatV<const c32>, bool, bool, bool, MatV<c32>);
template void ctrsm_dev<double>(MatV<const c64>, bool, bool, bool, MatV<c64>);

} // namespace fh
