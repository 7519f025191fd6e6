// Complex GEMM on the MFMA pipe (gfx950): dst(kind) <- [dst +] alpha * op(A) * op(B), op = identity or conjugate, for c32 / c64
// (interleaved {re, im}).  One kernel body, templated on the real type:
//   * operands are read interleaved from global memory (any element strides) and split into re / im planes on the way into LDS;
//   * a complex multiply-accumulate is the conventional four real MFMAs (never the 3M form: its error is not componentwise
//     bounded by |A||B|): re += Ar Br + Ai (-Bi), im += Ar Bi + Ai Br.  Conjugation is a sign flip of the im plane at the LDS
//     store, the minus of Im.Im a sign flip of the B fragment in registers;
//   * FaerBlock structure of lhs / rhs is a masked load (the excluded part is never read, a unit diagonal is supplied), DstKind and
//     the structure of dst a masked store.  No workspace: no split-K, no packing buffer.
#include <algorithm>

#include "common.h"
#include "mfma.h"

namespace fh {

namespace {

template <typename R> struct CGemmArgs {
	int M, N, K;
	Cx<R> *dst;
	idx_t drs, dcs;
	const Cx<R> *a;
	idx_t ars, acs; // element (m, k) at a[m * ars + k * acs]
	const Cx<R> *b;
	idx_t brs, bcs; // element (k, n) at b[k * brs + n * bcs]
	R alpha_re, alpha_im;
	int add;		// 1: dst += ; 0: dst = (dst is never read)
	int lower;		// 1: only i >= j written
	int dst_strict;		// lower: only i > j written
	int conj_a, conj_b;
	int a_struct, b_struct; // FaerBlock codes of lhs (m x k) and rhs (k x n)
	int akm, bkm;		// loader: consecutive threads walk along k (the operand's unit stride) instead of along m / n
	int a_vec, b_vec;	// the operand's elements are aligned to their own size: one vector load per element
	int ntm, ntn;
};

// FaerBlock membership test (faer/src/linalg/matmul/triangular.rs:906-977)
static __device__ __forceinline__ bool cx_in_block(int s, int i, int j)
{
	return s == 0 || ((s == 1) & (i >= j)) || ((s == 2) & (i <= j)) || (((s == 3) | (s == 5)) & (i > j)) ||
	       (((s == 4) | (s == 6)) & (i < j));
}

// hardware deals block b to XCD b % 8: give XCD x a contiguous range of logical ids (bijective for any grid size)
static __device__ __forceinline__ int cx_xcd_remap(int b, int nblocks)
{
	const int q = nblocks >> 3, r = nblocks & 7;
	const int xcd = b & 7, idx = b >> 3;
	return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

template <typename R> static __device__ __forceinline__ Cx<R> cx_load(const Cx<R> *p, int vec)
{
	typedef R v2 __attribute__((ext_vector_type(2)));
	if (vec) {
		const v2 t = *reinterpret_cast<const v2 *>(p);
		return Cx<R>{t.x, t.y};
	}
	return Cx<R>{p->re, p->im};
}

// 256 threads = 2 x 2 wavefronts; wave tile (BM / 2) x (BN / 2) in 16 x 16 MFMA fragments, two accumulator planes.
// LDS per stage: planes A_re, A_im (BK x (BM + 16)) and B_re, B_im (BK x (BN + 16)), k-major rows; two stages.
template <typename R, int BM, int BN, int BK>
__global__ __launch_bounds__(256, (BM == 128 ? 1 : 2)) void cgemm_kernel(const CGemmArgs<R> g)
{
	constexpr int NT = 256, WM = 2, WN = 2;
	constexpr int WTM = BM / WM, WTN = BN / WN;
	constexpr int TM = WTM / 16, TN = WTN / 16;
	constexpr int SA = BM + 16, SB = BN + 16;
	constexpr int A_PL = BK * SA, B_PL = BK * SB;
	constexpr int STAGE = 2 * (A_PL + B_PL);
	constexpr int A_CNT = BM * BK / NT, B_CNT = BN * BK / NT;
	static_assert(BM * BK % NT == 0 && BN * BK % NT == 0 && NT % BM == 0 && NT % BN == 0 && NT % BK == 0 && BK % 4 == 0, "tile/threads");
	typedef typename Mfma<R>::acc_t acc_t;

	extern __shared__ __align__(16) unsigned char cgemm_smem[];
	R *smem = reinterpret_cast<R *>(cgemm_smem);

	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int wm = wave % WM, wn = wave / WM;
	const int l15 = lane & 15, lhi = lane >> 4;

	int tm, tn;
	{
		const int pid = cx_xcd_remap(blockIdx.x, gridDim.x);
		constexpr int G = 8; // tile rows per raster group
		const int per_group = G * g.ntn;
		const int grp = pid / per_group;
		const int first_m = grp * G;
		const int gsz = min(g.ntm - first_m, G);
		const int rem = pid - grp * per_group;
		tm = first_m + rem % gsz;
		tn = rem / gsz;
	}
	const int m_off = tm * BM, n_off = tn * BN;
	if (g.lower && m_off + BM - 1 < n_off)
		return; // tile entirely above the diagonal

	// the K range outside which a triangular operand is identically zero for this tile
	int k_begin = 0, k_end = g.K;
	{
		const int as = g.a_struct, bs = g.b_struct;
		if (as == 1 || as == 3 || as == 5) // lhs lower: k <= m
			k_end = min(k_end, m_off + BM);
		if (as == 2 || as == 4 || as == 6) // lhs upper: k >= m
			k_begin = max(k_begin, m_off / BK * BK);
		if (bs == 1 || bs == 3 || bs == 5) // rhs lower: k >= n
			k_begin = max(k_begin, n_off / BK * BK);
		if (bs == 2 || bs == 4 || bs == 6) // rhs upper: k <= n
			k_end = min(k_end, n_off + BN);
	}
	const int nk = k_begin >= k_end ? 0 : (k_end - k_begin + BK - 1) / BK;
	if (nk == 0 && g.add)
		return; // nothing to accumulate (Replace still has to write zeros)

	// loader: element i of this thread is (mn + i * mstep, k + i * kstep), tile local
	const int a_mn = g.akm ? tid / BK : tid % BM, a_k = g.akm ? tid % BK : tid / BM;
	const int a_mstep = g.akm ? NT / BK : 0, a_kstep = g.akm ? 0 : NT / BM;
	const int b_mn = g.bkm ? tid / BK : tid % BN, b_k = g.bkm ? tid % BK : tid / BN;
	const int b_mstep = g.bkm ? NT / BK : 0, b_kstep = g.bkm ? 0 : NT / BN;

	Cx<R> ra[A_CNT], rb[B_CNT];

	auto load_a = [&](int k0) {
		const int as = g.a_struct;
#pragma unroll
		for (int i = 0; i < A_CNT; ++i) {
			const int mn = m_off + a_mn + i * a_mstep, k = k0 + a_k + i * a_kstep;
			const bool inside = mn < g.M && k < k_end;
			Cx<R> v{(R) 0, (R) 0};
			if (inside && cx_in_block(as, mn, k))
				v = cx_load(g.a + (idx_t) mn * g.ars + (idx_t) k * g.acs, g.a_vec);
			else if (inside && ((as == 5) | (as == 6)) && mn == k)
				v.re = (R) 1;
			if (g.conj_a)
				v.im = -v.im;
			ra[i] = v;
		}
	};
	auto load_b = [&](int k0) {
		const int bs = g.b_struct;
#pragma unroll
		for (int i = 0; i < B_CNT; ++i) {
			const int mn = n_off + b_mn + i * b_mstep, k = k0 + b_k + i * b_kstep;
			const bool inside = mn < g.N && k < k_end;
			Cx<R> v{(R) 0, (R) 0};
			if (inside && cx_in_block(bs, k, mn))
				v = cx_load(g.b + (idx_t) k * g.brs + (idx_t) mn * g.bcs, g.b_vec);
			else if (inside && ((bs == 5) | (bs == 6)) && mn == k)
				v.re = (R) 1;
			if (g.conj_b)
				v.im = -v.im;
			rb[i] = v;
		}
	};
	auto store_ab = [&](R *st) {
		R *sa = st, *sb = st + 2 * A_PL;
#pragma unroll
		for (int i = 0; i < A_CNT; ++i) {
			const int o = (a_k + i * a_kstep) * SA + a_mn + i * a_mstep;
			sa[o] = ra[i].re;
			sa[A_PL + o] = ra[i].im;
		}
#pragma unroll
		for (int i = 0; i < B_CNT; ++i) {
			const int o = (b_k + i * b_kstep) * SB + b_mn + i * b_mstep;
			sb[o] = rb[i].re;
			sb[B_PL + o] = rb[i].im;
		}
	};

	acc_t cre[TM][TN], cim[TM][TN];
#pragma unroll
	for (int i = 0; i < TM; ++i)
#pragma unroll
		for (int j = 0; j < TN; ++j) {
			cre[i][j] = (acc_t) (R) 0;
			cim[i][j] = (acc_t) (R) 0;
		}

	auto compute = [&](const R *st) {
		const R *sa = st, *sb = st + 2 * A_PL;
#pragma unroll
		for (int kk = 0; kk < BK / 4; ++kk) {
			R ar[TM], ai[TM], br[TN], bi[TN], nbi[TN];
#pragma unroll
			for (int i = 0; i < TM; ++i) {
				const int o = (kk * 4 + lhi) * SA + wm * WTM + i * 16 + l15;
				ar[i] = sa[o];
				ai[i] = sa[A_PL + o];
			}
#pragma unroll
			for (int j = 0; j < TN; ++j) {
				const int o = (kk * 4 + lhi) * SB + wn * WTN + j * 16 + l15;
				br[j] = sb[o];
				bi[j] = sb[B_PL + o];
				nbi[j] = -bi[j];
			}
			// (the MFMA's first operand indexes the result's register rows: n there, m along the lanes -- as in gemm.hip)
#pragma unroll
			for (int i = 0; i < TM; ++i)
#pragma unroll
				for (int j = 0; j < TN; ++j)
					cre[i][j] = Mfma<R>::run(br[j], ar[i], cre[i][j]);
#pragma unroll
			for (int i = 0; i < TM; ++i)
#pragma unroll
				for (int j = 0; j < TN; ++j)
					cim[i][j] = Mfma<R>::run(bi[j], ar[i], cim[i][j]);
#pragma unroll
			for (int i = 0; i < TM; ++i)
#pragma unroll
				for (int j = 0; j < TN; ++j)
					cre[i][j] = Mfma<R>::run(nbi[j], ai[i], cre[i][j]);
#pragma unroll
			for (int i = 0; i < TM; ++i)
#pragma unroll
				for (int j = 0; j < TN; ++j)
					cim[i][j] = Mfma<R>::run(br[j], ai[i], cim[i][j]);
		}
	};

	// K loop: iteration t multiplies tile t out of LDS stage t & 1 while the global loads of tile t + 1 are in flight; they land in
	// the other stage after the MFMA section.  One barrier per tile.  (Every load is bounds- and structure-checked.)
	if (nk > 0) {
		load_a(k_begin);
		load_b(k_begin);
		store_ab(smem);
	}
	__syncthreads();
	for (int kt = 0; kt < nk; ++kt) {
		const bool more = kt + 1 < nk;
		if (more) {
			load_a(k_begin + (kt + 1) * BK);
			load_b(k_begin + (kt + 1) * BK);
		}
		compute(smem + (kt & 1) * STAGE);
		if (more)
			store_ab(smem + ((kt + 1) & 1) * STAGE);
		__syncthreads();
	}

	// epilogue: lane (l15, lhi), register r of c??[i][j] holds C[m_off + wm*WTM + i*16 + l15][n_off + wn*WTN + j*16 + row(r, lhi)]
#pragma unroll
	for (int j = 0; j < TN; ++j)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int n = n_off + wn * WTN + j * 16 + Mfma<R>::row(r, lhi);
#pragma unroll
			for (int i = 0; i < TM; ++i) {
				const int m = m_off + wm * WTM + i * 16 + l15;
				const bool ok = n < g.N && m < g.M && !(g.lower && (m < n || (g.dst_strict && m == n)));
				if (!ok)
					continue;
				const R xr = cre[i][j][r], xi = cim[i][j][r];
				R vr = g.alpha_re * xr - g.alpha_im * xi, vi = g.alpha_re * xi + g.alpha_im * xr;
				Cx<R> *p = g.dst + (idx_t) m * g.drs + (idx_t) n * g.dcs;
				if (g.add) {
					vr += p->re;
					vi += p->im;
				}
				p->re = vr;
				p->im = vi;
			}
		}
}

template <typename R, int BM, int BN, int BK> void cgemm_launch(CGemmArgs<R> &g)
{
	g.ntm = (g.M + BM - 1) / BM;
	g.ntn = (g.N + BN - 1) / BN;
	constexpr size_t lds = (size_t) 2 * 2 * (BK * (BM + 16) + BK * (BN + 16)) * sizeof(R);
	static_assert(lds <= 160 * 1024, "LDS of a CU");
	raise_dynamic_lds<cgemm_kernel<R, BM, BN, BK>>(lds);
	hipLaunchKernelGGL((cgemm_kernel<R, BM, BN, BK>), dim3((unsigned) (g.ntm * g.ntn)), dim3(256), lds, ctx().stream, g);
	FH_HIP(hipGetLastError());
}

static inline idx_t iabs_(idx_t x) { return x < 0 ? -x : x; }

template <typename R>
void cgemm_dev(MatV<Cx<R>> C, DstKind kind, bool add, MatV<const Cx<R>> A, MatV<const Cx<R>> B, Cx<R> alpha, const GemmExtra<Cx<R>> *extra)
{
	FH_CHECK(A.nrows == C.nrows && B.ncols == C.ncols && A.ncols == B.nrows, "gemm: shape mismatch");
	GemmExtra<Cx<R>> ex;
	if (extra)
		ex = *extra;
	FH_CHECK(!ex.row_idx && !ex.col_idx && !ex.diag, "gemm: row_idx / col_idx / diag are not implemented for complex scalars (c32 / c64)");
	FH_CHECK(!ex.k_trim && !ex.tri_skip && !ex.stair_nb, "gemm: k_trim / tri_skip / stair_nb are real-scalar shortcuts");
	if (C.nrows == 0 || C.ncols == 0)
		return;
	if (A.ncols == 0 && add)
		return; // faer/src/linalg/matmul/mod.rs:1190-1198 (Replace: the kernel writes the zeros, through the same masked store)
	FH_CHECK(C.nrows < (1L << 30) && C.ncols < (1L << 30) && A.ncols < (1L << 30), "gemm: dimension too large");
	ctx().ensure_device();
	bool conj_a = ex.conj_lhs, conj_b = ex.conj_rhs;
	int a_s = ex.a_struct, b_s = ex.b_struct;
	// Upper(dst) == Lower(dst^T), dst^T = op(B)^T op(A)^T; a row-major Full dst is transposed too (unit dst stride along m)
	if (kind == DST_UPPER || (kind == DST_FULL && iabs_(C.cs) == 1 && iabs_(C.rs) != 1)) {
		static const int tr[7] = {0, 2, 1, 4, 3, 6, 5}; // FaerBlock of the transposed operand
		const MatV<const Cx<R>> At = B.t(), Bt = A.t();
		C = C.t();
		A = At;
		B = Bt;
		std::swap(conj_a, conj_b);
		const int as = tr[b_s], bs = tr[a_s];
		a_s = as;
		b_s = bs;
		if (kind == DST_UPPER)
			kind = DST_LOWER;
	}
	CGemmArgs<R> g;
	g.M = (int) C.nrows;
	g.N = (int) C.ncols;
	g.K = (int) A.ncols;
	g.dst = C.p;
	g.drs = C.rs;
	g.dcs = C.cs;
	g.a = A.p;
	g.ars = A.rs;
	g.acs = A.cs;
	g.b = B.p;
	g.brs = B.rs;
	g.bcs = B.cs;
	g.alpha_re = alpha.re;
	g.alpha_im = alpha.im;
	g.add = add;
	g.lower = kind == DST_LOWER;
	g.dst_strict = g.lower && ex.dst_strict;
	g.conj_a = conj_a;
	g.conj_b = conj_b;
	g.a_struct = a_s;
	g.b_struct = b_s;
	g.akm = iabs_(A.cs) == 1 && iabs_(A.rs) != 1;
	g.bkm = iabs_(B.rs) == 1 && iabs_(B.cs) != 1;
	g.a_vec = reinterpret_cast<uintptr_t>(A.p) % sizeof(Cx<R>) == 0;
	g.b_vec = reinterpret_cast<uintptr_t>(B.p) % sizeof(Cx<R>) == 0;
	// tile: c32 takes 128 x 128 (one workgroup per CU, twice the MFMAs per LDS byte) once that still fills the chip, else 64 x 64.
	// c64 stays at 64 x 64: the two accumulator planes of a 64 x 64 wave tile are 256 registers, and with the fragments and the
	// loader's prefetch the 128 x 128 tile spills (66 VGPRs at one wave per SIMD).
	const int variant = ctx().gemm_variant;
	const long tiles128 = ((long) (g.M + 127) / 128) * ((g.N + 127) / 128);
	bool big = sizeof(R) == 4 && tiles128 >= ctx().stream_cus();
	if (sizeof(R) == 4 && variant == GEMM_VARIANT_FORCE_128)
		big = true;
	if (variant == GEMM_VARIANT_FORCE_64)
		big = false;
	if constexpr (sizeof(R) == 4) {
		if (big) {
			cgemm_launch<R, 128, 128, 8>(g);
			return;
		}
	}
	cgemm_launch<R, 64, 64, sizeof(R) == 8 ? 8 : 16>(g);
}

template <typename R>
void cmatmul_triangular_dev(MatV<Cx<R>> C, int c_s, bool add, MatV<const Cx<R>> A, int a_s, MatV<const Cx<R>> B, int b_s, Cx<R> alpha)
{
	GemmExtra<Cx<R>> ex;
	ex.a_struct = a_s;
	ex.b_struct = b_s;
	DstKind kind = DST_FULL;
	if (c_s == 1 || c_s == 3 || c_s == 5)
		kind = DST_LOWER;
	else if (c_s == 2 || c_s == 4 || c_s == 6)
		kind = DST_UPPER;
	ex.dst_strict = c_s >= 3;
	cgemm_dev<R>(C, kind, add, A, B, alpha, &ex);
}

} // namespace

template <> void gemm_dev<c32>(MatV<c32> C, DstKind kind, bool add, MatV<const c32> A, MatV<const c32> B, c32 alpha, const GemmExtra<c32> *extra)
{
	cgemm_dev<float>(C, kind, add, A, B, alpha, extra);
}
template <> void gemm_dev<c64>(MatV<c64> C, DstKind kind, bool add, MatV<const c64> A, MatV<const c64> B, c64 alpha, const GemmExtra<c64> *extra)
{
	cgemm_dev<double>(C, kind, add, A, B, alpha, extra);
}
template <> void matmul_triangular_dev<c32>(MatV<c32> C, int c_s, bool add, MatV<const c32> A, int a_s, MatV<const c32> B, int b_s, c32 alpha)
{
	cmatmul_triangular_dev<float>(C, c_s, add, A, a_s, B, b_s, alpha);
}
template <> void matmul_triangular_dev<c64>(MatV<c64> C, int c_s, bool add, MatV<const c64> A, int a_s, MatV<const c64> B, int b_s, c64 alpha)
{
	cmatmul_triangular_dev<double>(C, c_s, add, A, a_s, B, b_s, alpha);
}

} // namespace fh
