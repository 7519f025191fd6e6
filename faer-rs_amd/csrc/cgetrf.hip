// Complex LU with partial pivoting for c32 / c64: getrf_dev<Cx<R>>.
//
// Driver: the reference's recursion (lu/partial_pivoting/factor.rs:68-222) on column ranges, halved down to panels of at most W
// columns.  Factor the left half, solve A01 <- L00^-1 A01 (ctrsm.hip), update A11 -= A10 A01 (one complex GEMM, cgemm.hip),
// recurse on the right half.  A panel applies its own interchanges to every column outside it as soon as it is factored -- the
// right-hand columns see the same transpositions in the same order as in the reference, before anything reads them.
//
// Panels (the hot path of this file), selected by height:
//   * clu_leaf_kernel: the panel lives in LDS as re / im planes, one workgroup runs all steps in one launch;
//   * clu_step_kernel: one launch per column for taller panels, any number of workgroups, no wait between workgroups: what one
//     launch needs from another workgroup (the pivot candidates, the candidate rows, the next diagonal row) was published to the
//     workspace by the launch before it.
// The arithmetic of a step is clu_core.h.  All device scratch is one Arena; nothing in it is read before it is written.
#include <algorithm>

#include "arena.h"
#include "clu_core.h"
#include "common.h"
#include "perm.h"

namespace fh {

namespace {

using namespace clu;

constexpr int W = 32;	     // panel width
constexpr int NT = 256;	     // threads of every kernel below
constexpr int MAX_WG = 1024; // workgroups of a column-step launch
// rows of the tallest panel the LDS leaf takes: two planes of W x rows reals, 128 KiB of the CU's 160
template <typename R> constexpr int leaf_rows() { return sizeof(R) == 4 ? 512 : 256; }

thread_local size_t g_clu_last[4] = {0, 0, 0, 0};

template <typename R> static __device__ __forceinline__ Cx<R> clu_ld(const Cx<R> *p, int vec)
{
	typedef R v2 __attribute__((ext_vector_type(2)));
	if (vec) {
		const v2 t = *reinterpret_cast<const v2 *>(p);
		return Cx<R>{t.x, t.y};
	}
	return Cx<R>{p->re, p->im};
}
template <typename R> static __device__ __forceinline__ void clu_st(Cx<R> *p, Cx<R> v, int vec)
{
	typedef R v2 __attribute__((ext_vector_type(2)));
	if (vec) {
		v2 t;
		t.x = v.re;
		t.y = v.im;
		*reinterpret_cast<v2 *>(p) = t;
	} else {
		p->re = v.re;
		p->im = v.im;
	}
}

// The workgroup's best (value, row): wave shuffle, then across the waves through LDS.  Every thread returns with the result.
// Two barriers; s_val / s_row may be reused after the next barrier of the caller.
template <typename R> static __device__ __forceinline__ void clu_wg_best(R &bv, int &br, R *s_val, int *s_row)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const R ov = __shfl_xor(bv, off, 64);
		const int orow = __shfl_xor(br, off, 64);
		clu_consider(ov, orow, bv, br);
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	__syncthreads(); // (the previous round's readers are done with s_val / s_row)
	if (lane == 0) {
		s_val[wave] = bv;
		s_row[wave] = br;
	}
	__syncthreads();
	bv = s_val[0];
	br = s_row[0];
#pragma unroll
	for (int k = 1; k < NT / 64; ++k)
		clu_consider(s_val[k], s_row[k], bv, br);
}

// ---- LDS-resident leaf: m x w panel (w <= W, w <= m <= leaf_rows), element (i, c) at plane[c * m + i]
template <typename R>
__global__ __launch_bounds__(NT) void clu_leaf_kernel(Cx<R> *A, idx_t rs, idx_t cs, int m, int w, int row_base, int *piv, int vec, int row_major)
{
	extern __shared__ __align__(16) unsigned char clu_smem[];
	R *pre = reinterpret_cast<R *>(clu_smem);
	R *pim = pre + (size_t) w * m;
	__shared__ R s_val[NT / 64];
	__shared__ int s_row[NT / 64];
	const int tid = threadIdx.x;
	const int total = m * w;
	for (int e = tid; e < total; e += NT) {
		const int i = row_major ? e / w : e % m, c = row_major ? e % w : e / m;
		const Cx<R> v = clu_ld(A + (idx_t) i * rs + (idx_t) c * cs, vec);
		pre[c * m + i] = v.re;
		pim[c * m + i] = v.im;
	}
	__syncthreads();
	const int nsteps = min(m, w);
	// this thread's candidate for the column about to be eliminated (rows ascending: the first of equal values stays)
	R bv = (R) 0;
	int br = 0;
	for (int i = tid; i < m; i += NT)
		clu_consider(clu_abs1(pre[i], pim[i]), i, bv, br);
	for (int j = 0; j < nsteps; ++j) {
		clu_wg_best(bv, br, s_val, s_row);
		const int p = br;
		if (tid == 0)
			piv[j] = row_base + p;
		if (p != j && tid < w) {
			R t = pre[tid * m + j];
			pre[tid * m + j] = pre[tid * m + p];
			pre[tid * m + p] = t;
			t = pim[tid * m + j];
			pim[tid * m + j] = pim[tid * m + p];
			pim[tid * m + p] = t;
		}
		__syncthreads();
		R ir, ii;
		clu_recip(pre[j * m + j], pim[j * m + j], ir, ii);
		bv = (R) 0;
		br = j + 1;
		for (int i = j + 1 + tid; i < m; i += NT) {
			R lr, li;
			clu_scale(pre[j * m + i], pim[j * m + i], ir, ii, lr, li);
			pre[j * m + i] = lr;
			pim[j * m + i] = li;
			for (int c = j + 1; c < w; ++c) {
				R xr = pre[c * m + i], xi = pim[c * m + i];
				clu_update(xr, xi, lr, li, pre[c * m + j], pim[c * m + j]);
				pre[c * m + i] = xr;
				pim[c * m + i] = xi;
				if (c == j + 1)
					clu_consider(clu_abs1(xr, xi), i, bv, br);
			}
		}
		__syncthreads();
	}
	for (int e = tid; e < total; e += NT) {
		const int i = row_major ? e / w : e % m, c = row_major ? e % w : e / m;
		clu_st(A + (idx_t) i * rs + (idx_t) c * cs, Cx<R>{pre[c * m + i], pim[c * m + i]}, vec);
	}
}

// ---- column-step panel: launch j = -1 (prologue), 0 .. w - 1.  Workgroup g owns rows [g * rpw, (g + 1) * rpw) of the panel.
// Workspace, double buffered by the parity of the column it is for:
//   cand_val / cand_row [2][nwg]     workgroup g's candidate for that column (value 0, row = the column: none found)
//   cand_rows           [2][nwg][W]  the candidate's whole panel row as the launch that found it left it
//   diag_rows           [2][W]       the panel row of that column's diagonal, likewise
// Launch j reads parity j & 1 and writes parity (j + 1) & 1, so no workgroup reads what another one of the same launch writes.
template <typename R> struct CStep {
	Cx<R> *A;
	idx_t rs, cs;
	int m, w, j, rpw, nwg, row_base, vec;
	R *cand_val;
	int *cand_row;
	Cx<R> *cand_rows, *diag_rows;
	int *piv;
};

template <typename R> __global__ __launch_bounds__(NT) void clu_step_kernel(const CStep<R> g)
{
	__shared__ R u_re[W], u_im[W], d_re[W], d_im[W];
	__shared__ R s_val[NT / 64];
	__shared__ int s_row[NT / 64];
	const int tid = threadIdx.x;
	const int j = g.j, jn = g.j + 1, w = g.w;
	const int r0 = blockIdx.x * g.rpw, r1 = min(g.m, r0 + g.rpw);
	// this thread's candidate for column jn among the rows of the workgroup
	R bv = (R) 0;
	int br = jn;
	if (j < 0) {
		for (int i = r0 + tid; i < r1; i += NT) {
			const Cx<R> v = clu_ld(g.A + (idx_t) i * g.rs, g.vec);
			clu_consider(clu_abs1(v.re, v.im), i, bv, br);
		}
	} else {
		// every workgroup reduces the candidates of the launch before: the pivot row p of column j
		const int par = j & 1;
		R pv = (R) 0;
		int p = j;
		for (int k = tid; k < g.nwg; k += NT)
			clu_consider(g.cand_val[par * g.nwg + k], g.cand_row[par * g.nwg + k], pv, p);
		clu_wg_best(pv, p, s_val, s_row);
		if (tid < w) {
			const Cx<R> d = g.diag_rows[par * W + tid];
			const Cx<R> u = p == j ? d : g.cand_rows[((size_t) par * g.nwg + p / g.rpw) * W + tid];
			u_re[tid] = u.re;
			u_im[tid] = u.im;
			d_re[tid] = d.re;
			d_im[tid] = d.im;
		}
		__syncthreads();
		if (blockIdx.x == 0 && tid == 0)
			g.piv[j] = g.row_base + p;
		// the interchange: the pivot row into slot j; slot p takes the old row j (below, as the source of its update)
		if (p != j && j >= r0 && j < r1 && tid < w)
			clu_st(g.A + (idx_t) j * g.rs + (idx_t) tid * g.cs, Cx<R>{u_re[tid], u_im[tid]}, g.vec);
		const bool own_p = p != j && p >= r0 && p < r1;
		R ir, ii;
		clu_recip(u_re[j], u_im[j], ir, ii);
		for (int i = max(r0, jn) + tid; i < r1; i += NT) {
			Cx<R> *row = g.A + (idx_t) i * g.rs;
			const bool from_d = own_p && i == p;
			Cx<R> a = from_d ? Cx<R>{d_re[j], d_im[j]} : clu_ld(row + (idx_t) j * g.cs, g.vec);
			R lr, li;
			clu_scale(a.re, a.im, ir, ii, lr, li);
			clu_st(row + (idx_t) j * g.cs, Cx<R>{lr, li}, g.vec);
			if (from_d)
				for (int c = 0; c < j; ++c)
					clu_st(row + (idx_t) c * g.cs, Cx<R>{d_re[c], d_im[c]}, g.vec);
			for (int c = jn; c < w; ++c) {
				Cx<R> x = from_d ? Cx<R>{d_re[c], d_im[c]} : clu_ld(row + (idx_t) c * g.cs, g.vec);
				clu_update(x.re, x.im, lr, li, u_re[c], u_im[c]);
				clu_st(row + (idx_t) c * g.cs, x, g.vec);
				if (c == jn)
					clu_consider(clu_abs1(x.re, x.im), i, bv, br);
			}
		}
	}
	if (jn >= w)
		return; // the last column: nothing to publish
	__threadfence_block();
	clu_wg_best(bv, br, s_val, s_row); // (its barriers also order the row stores above before the reads below)
	const int npar = jn & 1;
	if (tid == 0) {
		g.cand_val[npar * g.nwg + blockIdx.x] = bv;
		g.cand_row[npar * g.nwg + blockIdx.x] = br;
	}
	if (tid < w && br >= r0 && br < r1)
		g.cand_rows[((size_t) npar * g.nwg + blockIdx.x) * W + tid] = clu_ld(g.A + (idx_t) br * g.rs + (idx_t) tid * g.cs, g.vec);
	if (tid < w && jn >= r0 && jn < r1)
		g.diag_rows[npar * W + tid] = clu_ld(g.A + (idx_t) jn * g.rs + (idx_t) tid * g.cs, g.vec);
}

// ---- interchanges of one panel on the columns outside it: the nt <= W transpositions (j <-> piv[j] - row_base) composed once into a
// move list of at most 2 nt rows (dst[e] takes the row that was at src[e]; src[e] < 0: nothing to do) ...
__global__ __launch_bounds__(64) void clu_compose_kernel(const int *__restrict__ piv, int nt, int row_base, int *dst, int *src)
{
	__shared__ int s_piv[W];
	const int e = threadIdx.x;
	if (e < nt)
		s_piv[e] = piv[e] - row_base;
	__syncthreads();
	if (e >= 2 * nt)
		return;
	const int d = e < nt ? e : s_piv[e - nt];
	int pos = -1;
	if (e < nt || d >= nt) {
		pos = d;
		for (int j = nt - 1; j >= 0; --j) {
			const int pj = s_piv[j];
			pos = pos == j ? pj : (pos == pj ? j : pos);
		}
		if (pos == d)
			pos = -1;
	}
	dst[e] = d;
	src[e] = pos;
}
// ... and applied: 64 list entries x 4 columns per workgroup, all loads of a column before its stores.  Column c of the launch is
// column c of B for c < skip0 and column c + skipw from there on (the panel's own columns are left out).
template <typename R>
__global__ __launch_bounds__(NT) void clu_swap_kernel(Cx<R> *B, idx_t rs, idx_t cs, int ncols, int skip0, int skipw, const int *__restrict__ dst,
						      const int *__restrict__ src, int ne, int vec)
{
	const int e = threadIdx.x & 63;
	const int c = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
	const bool active = e < ne && c < ncols;
	const int sr = active ? src[e] : -1;
	const idx_t col = (idx_t) (c < skip0 ? c : c + skipw) * cs;
	Cx<R> v{(R) 0, (R) 0};
	if (sr >= 0)
		v = clu_ld(B + (idx_t) sr * rs + col, vec);
	__syncthreads();
	if (sr >= 0)
		clu_st(B + (idx_t) dst[e] * rs + col, v, vec);
}

inline idx_t cdiv(idx_t a, idx_t b) { return (a + b - 1) / b; }
// rows per workgroup of a column-step panel of mp rows: a multiple of NT, at most MAX_WG workgroups
inline idx_t step_rpw(idx_t mp) { return NT * cdiv(mp, (idx_t) NT * MAX_WG); }

template <typename R> struct Clu {
	MatV<Cx<R>> A;
	int vec;
	int *piv;  // min(m, n): absolute pivot rows
	R *cand_val;
	int *cand_row;
	Cx<R> *cand_rows, *diag_rows;
	int *list; // dst[2 W], src[2 W]

	static size_t plan(idx_t m, idx_t n)
	{
		const size_t k = (size_t) std::min(m, n), nwg = (size_t) std::min<idx_t>(MAX_WG, cdiv(m, NT));
		return Arena::padded(k * sizeof(int)) + Arena::padded(2 * nwg * sizeof(R)) + Arena::padded(2 * nwg * sizeof(int)) +
		       Arena::padded(2 * nwg * W * sizeof(Cx<R>)) + Arena::padded(2 * W * sizeof(Cx<R>)) + Arena::padded(4 * W * sizeof(int));
	}
	Clu(Arena &ar, MatV<Cx<R>> A_) : A(A_)
	{
		const size_t k = (size_t) std::min(A.nrows, A.ncols), nwg = (size_t) std::min<idx_t>(MAX_WG, cdiv(A.nrows, NT));
		vec = reinterpret_cast<uintptr_t>(A.p) % sizeof(Cx<R>) == 0;
		piv = ar.take<int>(k);
		cand_val = ar.take<R>(2 * nwg);
		cand_row = ar.take<int>(2 * nwg);
		cand_rows = ar.take<Cx<R>>(2 * nwg * W);
		diag_rows = ar.take<Cx<R>>(2 * W);
		list = ar.take<int>(4 * W);
	}

	// columns [c0, c0 + w) of rows [c0, m), then the panel's interchanges on all other columns of those rows
	void panel(idx_t c0, idx_t w)
	{
		hipStream_t s = ctx().stream;
		const idx_t mp = A.nrows - c0;
		MatV<Cx<R>> P = A.sub(c0, c0, mp, w);
		auto ab = [](idx_t x) { return x < 0 ? -x : x; };
		if (mp <= leaf_rows<R>()) {
			const size_t lds = (size_t) 2 * w * mp * sizeof(R);
			raise_dynamic_lds<clu_leaf_kernel<R>>((size_t) 2 * W * leaf_rows<R>() * sizeof(R));
			hipLaunchKernelGGL(clu_leaf_kernel<R>, dim3(1), dim3(NT), lds, s, P.p, P.rs, P.cs, (int) mp, (int) w, (int) c0, piv + c0, vec,
					   (int) (ab(P.cs) < ab(P.rs)));
			FH_HIP(hipGetLastError());
			++g_clu_last[0];
		} else {
			CStep<R> g;
			g.A = P.p;
			g.rs = P.rs;
			g.cs = P.cs;
			g.m = (int) mp;
			g.w = (int) w;
			g.rpw = (int) step_rpw(mp);
			g.nwg = (int) cdiv(mp, g.rpw);
			g.row_base = (int) c0;
			g.vec = vec;
			g.cand_val = cand_val;
			g.cand_row = cand_row;
			g.cand_rows = cand_rows;
			g.diag_rows = diag_rows;
			g.piv = piv + c0;
			for (int j = -1; j < (int) w; ++j) {
				g.j = j;
				hipLaunchKernelGGL(clu_step_kernel<R>, dim3((unsigned) g.nwg), dim3(NT), 0, s, g);
				FH_HIP(hipGetLastError());
			}
			++g_clu_last[1];
			g_clu_last[2] += (size_t) w + 1;
		}
		const idx_t others = A.ncols - w;
		if (others == 0 || mp < 2)
			return;
		hipLaunchKernelGGL(clu_compose_kernel, dim3(1), dim3(64), 0, s, piv + c0, (int) w, (int) c0, list, list + 2 * W);
		FH_HIP(hipGetLastError());
		MatV<Cx<R>> B = A.sub(c0, 0, mp, A.ncols);
		hipLaunchKernelGGL(clu_swap_kernel<R>, dim3((unsigned) cdiv(others, NT / 64)), dim3(NT), 0, s, B.p, B.rs, B.cs, (int) others, (int) c0, (int) w,
				   list, list + 2 * W, (int) (2 * w), vec);
		FH_HIP(hipGetLastError());
		++g_clu_last[3];
	}

	// columns [c0, c0 + nc) of rows [c0, m), nc <= m - c0
	void rec(idx_t c0, idx_t nc)
	{
		if (nc <= W) {
			panel(c0, nc);
			return;
		}
		const idx_t h = cdiv(nc / 2, W) * W; // W <= h < nc
		const idx_t m = A.nrows;
		rec(c0, h);
		MatV<Cx<R>> A01 = A.sub(c0, c0 + h, h, nc - h);
		ctrsm_dev<R>(A.sub(c0, c0, h, h).c(), false, true, false, A01);
		if (m > c0 + h)
			gemm_dev<Cx<R>>(A.sub(c0 + h, c0 + h, m - c0 - h, nc - h), DST_FULL, true, A.sub(c0 + h, c0, m - c0 - h, h).c(), A01.c(),
					Cx<R>{(R) -1, (R) 0});
		rec(c0 + h, nc - h);
	}
};

template <typename R> long cgetrf(MatV<Cx<R>> A, idx_t *perm, idx_t *perm_inv)
{
	const idx_t m = A.nrows, n = A.ncols, k = std::min(m, n);
	for (size_t i = 0; i < 4; ++i)
		g_clu_last[i] = 0;
	if (k == 0) {
		for (idx_t i = 0; i < m; ++i)
			perm[i] = perm_inv[i] = i;
		return 0;
	}
	FH_CHECK(m < (1L << 30) && n < (1L << 30), "partial_piv_lu: dimension too large");
	ctx().ensure_device();
	std::vector<int> piv((size_t) k);
	{
		Arena arena(Clu<R>::plan(m, n));
		Clu<R> f(arena, A);
		f.rec(0, k);
		if (n > k) // wide: the columns right of the square part (their rows are interchanged already)
			ctrsm_dev<R>(A.sub(0, 0, k, k).c(), false, true, false, A.sub(0, k, k, n - k));
		// the pivot records come back once per call
		FH_HIP(hipMemcpyAsync(piv.data(), f.piv, (size_t) k * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
		ctx().sync();
	}
	return perm_from_transpositions("partial_piv_lu", m, k, [&](idx_t j) { return (idx_t) piv[(size_t) j]; }, perm, perm_inv);
}

} // namespace

void clu_shape(int elem_bytes, size_t out[2])
{
	out[0] = W;
	out[1] = elem_bytes == 16 ? leaf_rows<double>() : leaf_rows<float>();
}
void clu_last(size_t out[4])
{
	for (size_t i = 0; i < 4; ++i)
		out[i] = g_clu_last[i];
}

template <> long getrf_dev<c32>(MatV<c32> A, idx_t *perm, idx_t *perm_inv) { return cgetrf<float>(A, perm, perm_inv); }
template <> long getrf_dev<c64>(MatV<c64> A, idx_t *perm, idx_t *perm_inv) { return cgetrf<double>(A, perm, perm_inv); }

} // namespace fh
