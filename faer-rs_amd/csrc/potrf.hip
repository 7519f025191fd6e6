// In-place lower Cholesky (LLT) for gfx950.
//
// Replaces faer/src/linalg/cholesky/llt/factor.rs:67-97 and the engine behind it,
// cholesky/ldlt/factor.rs:7-498.
//
// The reference is right-looking with 128-column steps (factor.rs:392).  A rank-128 fp64 update is only
// ~16 flop/byte -- at the MI355X machine balance -- so the GPU drivers use larger steps with the same arithmetic per
// entry: recursion by HALVES below 2048 columns (potrf_rec), 1024-column steps above (potrf_lookahead: right-looking
// panels in 128-column blocks, trailing updates with K = 1024, look-ahead on two CU-masked streams for large n).
//
// Leaf (n <= 128): ONE 512-thread workgroup, the block resident in LDS (lds_blocks.h), blocked right-looking
// in four 32-column steps:
//   * panel step: the 32 x 32 diagonal block and the rows below it are factored by up to three wavefronts
//     WITHOUT any synchronisation inside the step: every wavefront keeps the diagonal block's rows in lanes
//     0-31 (redundantly) and 32 of the rows below in lanes 32-63, one matrix row per lane in 32 registers; the
//     multipliers l_kj reach the other lanes through v_readlane.  The per-column dependency chain
//     (sqrt -> reciprocal -> scale -> update of the next diagonal entry) is the only serial part;
//   * trailing step: A22 -= L21 L21^T on the MFMA pipe straight out of LDS (K = 32, 16 x 16 tiles over 8 waves);
//   * semantics of the reference's base kernel (factor.rs:122-174): d = a_jj (optionally regularised and
//     counted), fail with the GLOBAL column index if !(d > 0), every entry of column j -- the diagonal one
//     included -- is multiplied by the reciprocal 1 / sqrt(d).
// The leaf also writes the PACKED IMAGE of its L_kk (trsm_pack.h) into the factorization's workspace: the panel
// solves of all enclosing levels substitute against it (trsm_lower_pre_dev: substitution inside the 128-blocks like
// the reference's triangular_solve.rs, MFMA products off the diagonal) without a separate packing launch.
// Failure is reported through a device status word (first failing GLOBAL column index + 1); later
// kernels see it and become no-ops, so the host synchronises exactly once per factorization.
#include "common.h"
#include "lds_blocks.h"
#include "trsm_pack.h"

namespace fh {

constexpr int POTRF_NB = LDS_NB;
constexpr int POTRF_PB = 32; // panel width inside the leaf

// inv = 1 / sqrt(d) for a wave-uniform d > 0 on the shortest dependent chain: v_rsq_f64, one coupled Newton
// step for (g ~ sqrt d, h ~ 1 / (2 sqrt d)) and one more step for h: 7 dependent operations instead of the
// ~25 of sqrt() followed by a division.  This chain is the serial part of the leaf (128 dependent columns);
// the result is within an ulp or two of the reference's (1 / sqrt(d)) (cholesky/ldlt/factor.rs:160-163), well
// inside the parity tolerance.  Outside a safe exponent range it falls back to the library sqrt and division.
// Returns false for the reference's failure cases (!(d > 0), sqrt not finite or zero).
static __device__ __forceinline__ bool recip_sqrt(double d, double &inv)
{
	if (d > 1e-280 && d < 1e280) {
		const double y = __builtin_amdgcn_rsq(d);
		double g = d * y, h = 0.5 * y;
		double r = fh_fma(-h, g, 0.5);
		g = fh_fma(g, r, g);
		h = fh_fma(h, r, h);
		r = fh_fma(-h, g, 0.5);
		h = fh_fma(h, r, h);
		inv = h + h;
		return true;
	}
	const double sq = sqrt(d);
	inv = 1.0 / sq;
	return d > 0.0 && sq != 0.0 && isfinite(sq);
}
static __device__ __forceinline__ bool recip_sqrt(float d, float &inv)
{
	const float sq = sqrtf(d);
	inv = 1.0f / sq;
	return d > 0.0f && sq != 0.0f && isfinite(sq);
}

#ifdef FH_LEAF_TIMING
#define FH_LT(i)                                                                                                         \
	do {                                                                                                             \
		const long long now_ = (long long) __builtin_readcyclecounter();                                         \
		tacc[i] += now_ - tlast;                                                                                 \
		tlast = now_;                                                                                            \
	} while (0)
__device__ unsigned long long g_leaf_timing[8];
#else
#define FH_LT(i)                                                                                                         \
	do {                                                                                                             \
	} while (0)
#endif

// LDLT == true: the same leaf for the unit-lower L D L^T factorization (cholesky/ldlt/factor.rs with is_llt ==
// false): the pivot d_j is kept (no root), regularised according to its expected sign, a zero / non finite pivot
// is the error, the column is divided by d_j, the updates are weighted by d_j, D goes to `Dout` and -- like the
// reference's cholesky_in_place (:791-798) -- onto the diagonal of A.
template <typename T, bool LDLT>
__global__ __launch_bounds__(LDS_NT) void potrf_leaf_kernel(T *A, idx_t rs, idx_t cs, int n, int regularize, T eps, T delta,
							   int *status, int offset, T *Winv, const signed char *signs, T *Dout)
{
	__shared__ T S[LDS_NB * LDS_LDP];
	__shared__ T s_d[LDS_NB]; // LDLT: the pivots of this block
	__shared__ int s_fail;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (status[0] != 0)
		return; // an earlier block already failed
	if (tid == 0)
		s_fail = 0;
#ifdef FH_LEAF_TIMING
	long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	long long tlast = (long long) __builtin_readcyclecounter();
#endif
	lds_load_lower<T>(S, A, rs, cs, n);
	__syncthreads();
	FH_LT(0);

	const int np = (n + POTRF_PB - 1) / POTRF_PB * POTRF_PB; // identity padded
	int count = 0;
	bool failed = false;
	for (int j0 = 0; j0 < np; j0 += POTRF_PB) {
		// ---- panel step: rows j0 .. np-1 of columns j0 .. j0+31
		const int below = np - j0 - POTRF_PB; // rows under the diagonal block (multiple of 32)
		const int nw = below > 0 ? below / 32 : 1;
		// every panel wave first LOADS its rows (the diagonal block's rows are loaded by all of them), and only after
		// a workgroup barrier do the waves start writing finished columns back into the block image: without it
		// a wave that runs ahead overwrites diagonal-block entries that a slower wave has not loaded yet (seen as
		// rare spurious failures once other kernels shared the chip and skewed the waves)
		const bool diag_lane = lane < 32;
		const int row = diag_lane ? j0 + lane : j0 + POTRF_PB + wave * 32 + (lane - 32);
		const bool valid = row < np;
		T a[POTRF_PB];
		if (wave < nw) {
			const int rr = valid ? row : j0;
#pragma unroll
			for (int c = 0; c < POTRF_PB; ++c)
				a[c] = S[(j0 + c) * LDS_LDP + rr];
		}
		__syncthreads();
		if (wave < nw) {
			int fail_col = 0;
			// the reciprocal root of column j is computed one iteration ahead, right after the diagonal entry
			// a_jj has received its last update through the register path, so that the long latencies
			// (rsq chain, LDS round trip of the multipliers) overlap instead of adding up
			T inv, dj = (T) 1; // dj: the pivot of the current column (LDLT)
			bool ok;
			// pivot of column jc from its updated diagonal entry d: regularisation (cholesky/ldlt/factor.rs:122-144;
			// llt: sign == +1, only that correction is counted), then 1/sqrt(d) (LLT) or 1/d (LDLT)
			auto pivot = [&](T d, int jc, T &inv_out, T &d_out) -> bool {
				if (regularize) {
					if constexpr (LDLT) {
						const int sign = (signs && jc < n) ? (int) signs[offset + jc] : 0;
						const bool small_or_negative = d <= eps, minus_small_or_positive = d >= -eps;
						if (sign == 1 && small_or_negative) {
							d = delta;
							if (jc < n)
								++count;
						} else if (sign == -1 && minus_small_or_positive) {
							d = -delta;
						} else if (small_or_negative && minus_small_or_positive) {
							d = d < (T) 0 ? -delta : delta;
						}
					} else if (d <= eps) {
						d = delta;
						if (jc < n)
							++count;
					}
				}
				d_out = d;
				if constexpr (LDLT) {
					inv_out = (T) 1 / d;
					return d != (T) 0 && isfinite(d);
				} else {
					return recip_sqrt(d, inv_out);
				}
			};
			ok = pivot(lane_bcast(a[0], 0), j0, inv, dj);
#pragma unroll
			for (int j = 0; j < POTRF_PB; ++j) {
				if (fail_col == 0) { // wave uniform
					if (!ok) {
						fail_col = j0 + j + 1;
						if (LDLT && wave == 0 && lane == 0)
							s_d[j0 + j] = dj; // the failing pivot still goes to D (factor.rs:343-347, :791-798)
					} else {
						const T lj = a[j] * inv; // column j, diagonal entry included (factor.rs:160-174)
						const T wj = LDLT ? dj : (T) 1; // weight of column j in the updates: a_ik -= l_ij d_j l_kj
						// column j is final: park it in the block image (every panel wave writes the same
						// diagonal-block values); the multipliers l_kj, k >= j + 2, come back as broadcast reads
						// (LDS operations of one wavefront execute in order)
						T *colj = S + (j0 + j) * LDS_LDP;
						if (valid && (!diag_lane || lane >= j))
							colj[row] = lj;
						if (LDLT && wave == 0 && lane == 0)
							s_d[j0 + j] = dj;
						__builtin_amdgcn_wave_barrier();
						T mult[POTRF_PB];
#pragma unroll
						for (int k = j + 2; k < POTRF_PB; ++k)
							mult[k] = colj[j0 + k] * wj;
						if (j + 1 < POTRF_PB) {
							// critical path: next diagonal entry through v_readlane, then its pivot
							a[j + 1] = fh_fma(-lj, lane_bcast(lj, j + 1) * wj, a[j + 1]);
							ok = pivot(lane_bcast(a[j + 1], j + 1), j0 + j + 1, inv, dj);
						}
#pragma unroll
						for (int k = j + 2; k < POTRF_PB; ++k)
							a[k] = fh_fma(-lj, mult[k], a[k]); // a_ik -= l_ij (d_j) l_kj
					}
				}
			}
			if (fail_col != 0 && tid == 0)
				s_fail = fail_col;
		}
		__syncthreads();
		FH_LT(1);
		if (s_fail != 0) {
			failed = true;
			break;
		}
		// ---- trailing step: A22(lower) -= L21 L21^T, L21 = rows j0+32 .. np-1 of the panel (K = 32)
		if (below > 0) {
			const int nt = below / 16;
			const int ntiles = nt * (nt + 1) / 2;
			const int l15 = lane & 15, lhi = lane >> 4;
			const int t0 = j0 + POTRF_PB;
			for (int t = wave; t < ntiles; t += LDS_NW) {
				// t enumerates (ti >= tj) row by row
				int ti = (int) ((sqrtf(8.0f * (float) t + 1.0f) - 1.0f) * 0.5f);
				while ((ti + 1) * (ti + 2) / 2 <= t)
					++ti;
				while (ti * (ti + 1) / 2 > t)
					--ti;
				const int tj = t - ti * (ti + 1) / 2;
				// D[i][j] = sum_k L[t0 + 16 ti + i][k] L[t0 + 16 tj + j][k]: A-type reads for both operands
				typename Mfma<T>::acc_t acc = (typename Mfma<T>::acc_t) (T) 0;
				const T *pa = S + (j0 + lhi) * LDS_LDP + t0 + ti * 16 + l15;
				const T *pb = S + (j0 + lhi) * LDS_LDP + t0 + tj * 16 + l15;
#pragma unroll
				for (int kk = 0; kk < POTRF_PB; kk += 4)
					acc = Mfma<T>::run(pa[kk * LDS_LDP], LDLT ? pb[kk * LDS_LDP] * s_d[j0 + kk + lhi] : pb[kk * LDS_LDP], acc);
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const int gi = t0 + ti * 16 + Mfma<T>::row(r, lhi), gj = t0 + tj * 16 + l15;
					if (gi >= gj)
						S[gj * LDS_LDP + gi] -= acc[r];
				}
			}
		}
		__syncthreads();
		FH_LT(2);
	}
	// ---- write back the lower triangle (also after a failure: the columns before the failing one are final)
	if constexpr (LDLT) {
		// D for the columns 0 .. index (cholesky/ldlt/factor.rs:791-798), both on the diagonal of A and in Dout
		const int init = failed ? s_fail : n;
		__syncthreads();
		if (tid < n && tid < init) {
			S[tid * LDS_LDP + tid] = s_d[tid];
			Dout[offset + tid] = s_d[tid];
		}
		__syncthreads();
	}
	lds_store_block<T>(S, A, rs, cs, n, true);
	FH_LT(3);
	if (failed) {
		if (tid == 0)
			atomicCAS(status, 0, offset + s_fail);
		return;
	}
	if (tid == 0 && count > 0)
		atomicAdd(status + 1, count);
	if (Winv) {
		// packed image of L_kk for the substitution leaf of the panel solves (unit diagonal for LDLT)
		typedef TriPack<T> P;
		for (int e = tid; e < TP_NT * P::DG_SZ; e += LDS_NT) // alignment holes of the diagonal tiles
			Winv[P::OFF_DG + e] = (T) 0;
		__syncthreads();
		for (int e = tid; e < LDS_NB * LDS_NB; e += LDS_NT) {
			const int i = e % LDS_NB, j = e / LDS_NB;
			if (j > i)
				continue;
			const T v = S[j * LDS_LDP + i];
			bool neg;
			const int ps = P::pos(i, j, neg);
			const T val = i == j ? ((LDLT || i >= n) ? (T) 1 : (T) 1 / v) : v; // the diagonal enters as its reciprocal
			Winv[ps] = neg ? -val : val;
		}
		FH_LT(4);
	}
#ifdef FH_LEAF_TIMING
	if (tid == 0)
		for (int i = 0; i < 8; ++i)
			atomicAdd(&g_leaf_timing[i], (unsigned long long) tacc[i]);
#endif
}

// What the levels of one factorization share: regularisation rule, device status word, the packed images of the diagonal blocks
template <typename T> struct CholWork {
	int regularize;
	T eps, delta;
	int *status;			    // [0] first failing global column + 1, [1] regularisation count
	T *Wbase;			    // one image per 128-block
	idx_t wblk0 = 0;		    // the 128-block whose image is slot 0 (potrf_panel_dev: the panel's first one)
	const signed char *signs = nullptr; // LDLT: expected pivot signs (null: none given)
	T *Dv = nullptr;		    // LDLT: the pivots
	// the image of the 128-block that starts at global column j
	T *wslot(idx_t j) const { return Wbase + (size_t) (j / POTRF_NB - wblk0) * TriPack<T>::SIZE; }
};

// the leaf on the diagonal block D (<= 128 columns, at global column `offset`); W: where its packed image goes (null: no
// solve will read it).  The LLT leaves are kernel class 5 of the profile, the LDLT leaf is not profiled.
template <typename T, bool LDLT> static void chol_leaf(MatV<T> D, idx_t offset, T *W, const CholWork<T> &wk)
{
	ProfScope prof(LDLT ? -1 : 5, (double) D.nrows);
	hipLaunchKernelGGL((potrf_leaf_kernel<T, LDLT>), dim3(1), dim3(LDS_NT), 0, ctx().stream, D.p, D.rs, D.cs, (int) D.nrows, wk.regularize,
			   wk.eps, wk.delta, wk.status, (int) offset, W, wk.signs, wk.Dv);
	FH_HIP(hipGetLastError());
}

// X[:, k] /= d[k]  (LDLT: A10 <- L10 = A10 D0^-1, cholesky/ldlt/factor.rs:447-455)
template <typename T> __global__ void scale_cols_recip_kernel(T *X, idx_t rs, idx_t cs, idx_t m, idx_t n, const T *__restrict__ d)
{
	const idx_t total = m * n;
	for (idx_t e = (idx_t) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (idx_t) gridDim.x * blockDim.x) {
		const idx_t i = e % m, k = e / m;
		X[i * rs + k * cs] *= (T) 1 / d[k];
	}
}

// Recursion by halves, for L L^T and for L D L^T (unit lower L, diagonal D, no pivoting: cholesky/ldlt/factor.rs:367-498 with
// is_llt == false).  LDLT differs in the leaf, and in that the panel solve -- against the unit
// triangles -- leaves L10 D0: A10 is then scaled by 1 / D0 (:447-455) and the trailing update is the diagonally weighted
// product of the spicy_matmul surface (:456-470), lower(A11) -= L10 D0 L10^T.
template <typename T, bool LDLT> static void chol_rec(MatV<T> A, const CholWork<T> &wk, idx_t offset, bool need_inv)
{
	const idx_t n = A.nrows;
	if (n == 0)
		return;
	if (n <= POTRF_NB) {
		chol_leaf<T, LDLT>(A, offset, need_inv ? wk.wslot(offset) : nullptr, wk);
		return;
	}
	const idx_t h = ((n / 2 + POTRF_NB - 1) / POTRF_NB) * POTRF_NB;
	MatV<T> A00 = A.sub(0, 0, h, h), A10 = A.sub(h, 0, n - h, h), A11 = A.sub(h, h, n - h, n - h);
	chol_rec<T, LDLT>(A00, wk, offset, true);
	// A10 <- A10 L00^-T, expressed like the reference (cholesky/ldlt/factor.rs:422-426) as L00 \ A10^T
	trsm_lower_pre_dev<T>(A00.c(), A10.t(), wk.wslot(offset));
	GemmExtra<T> ex;
	if constexpr (LDLT) {
		const idx_t total = (n - h) * h;
		idx_t blocks = (total + 255) / 256;
		if (blocks > 65536)
			blocks = 65536;
		hipLaunchKernelGGL(scale_cols_recip_kernel<T>, dim3((unsigned) blocks), dim3(256), 0, ctx().stream, A10.p, A10.rs, A10.cs, n - h, h,
				   wk.Dv + offset);
		FH_HIP(hipGetLastError());
		ex.diag = wk.Dv + offset;
		ex.diag_stride = 1;
	}
	// lower(A11) -= A10 [D0] A10^T  (cholesky/ldlt/factor.rs:436-446 -> triangular.rs:602 DstKind::Lower)
	gemm_dev<T>(A11, DST_LOWER, true, A10.c(), A10.t().c(), (T) -1, LDLT ? &ex : nullptr);
	chol_rec<T, LDLT>(A11, wk, offset + h, need_inv);
}

// Factorization of a tall panel P (R x w, R >= w; the top w x w block is the diagonal block) in 128-column blocks -- three
// launches per block on ONE dependent chain, right-looking like the reference's own sweep (cholesky/ldlt/factor.rs:367-498
// with its 128-column step, :392):
//     leaf on the diagonal block                               (also yields the packed image W_j of L_jj)
//     rows below      <-  rows below * L_jj^-T                 (substitution leaf against W_j, trsm.hip)
//     panel right of block j  -=  P[c1:, j] P[c1:w, j]^T       (lower trapezoid, ONE GEMM with K = 128)
// instead of the ~38 launches of the recursion above for 8 blocks.  Used where the diagonal-block chain is the critical
// path (look-ahead panel stream, the sequential tail, the distributed driver's panels).
// Rounds 2-4 ran this LEFT-looking (block column j -= P[c0:, 0:c0] P[c0:c0+128, 0:c0]^T before its leaf, K = c0): on the 32
// reserved CUs those launches were 15-59 us (a K = 896 product on a 128-column output has 4-16 workgroups), the K = 128
// trapezoids are 12-25 us.  Measured (profiles/r05_exp_llt_driver.txt): N = 16384 34.7-35.0 -> 34.0-34.1 ms, N = 8192 10.4-11.5
// -> 9.6-9.7 ms; with the cheaper diagonal chains the look-ahead steps beat the sequential tail down to 1024 rows: 33.2 ms.
template <typename T, typename AfterBlock>
static void potrf_panel_flat_hook(MatV<T> P, const CholWork<T> &wk, idx_t offset, AfterBlock after_block)
{
	const idx_t R = P.nrows, w = P.ncols;
	for (idx_t c0 = 0; c0 < w; c0 += POTRF_NB) {
		const idx_t nb = POTRF_NB < w - c0 ? POTRF_NB : w - c0;
		T *W = wk.wslot(offset + c0);
		MatV<T> D = P.sub(c0, c0, nb, nb);
		chol_leaf<T, false>(D, offset + c0, W, wk);
		if (R > c0 + nb) // rows below <- rows below * L_kk^-T: substitution leaf, lanes along the rows of the panel
			trsm_lower_pre_dev<T>(D.c(), P.sub(c0 + nb, c0, R - c0 - nb, nb).t(), W);
		after_block(c0, nb, W); // (block column c0 of L is final, the packed image of its diagonal block is in W)
		if (c0 + nb < w) {
			const idx_t c1 = c0 + nb;
			gemm_dev<T>(P.sub(c1, c1, R - c1, w - c1), DST_LOWER, true, P.sub(c1, c0, R - c1, nb).c(), P.sub(c1, c0, w - c1, nb).t().c(), (T) -1);
		}
	}
}
template <typename T> static void potrf_panel_flat(MatV<T> P, const CholWork<T> &wk, idx_t offset)
{
	potrf_panel_flat_hook<T>(P, wk, offset, [](idx_t, idx_t, T *) {});
}

// Right-looking driver with look-ahead for large matrices: steps of LA_NB columns,
//     [panel stream]  D_k = chol(A_kk)                         (flat panel above; latency bound, few CUs)
//     [bulk stream]   P_k = A_{>k,k} L_kk^-T                   (in place: substitution leaves + MFMA products)
//     [bulk stream]   A_{k+1,k+1} -= P_k[0] P_k[0]^T           -> releases D_{k+1} on the panel stream
//     [bulk stream]   rest of the trailing matrix -= P_k P_k^T (K = LA_NB: compute bound)
// The diagonal-block factorizations -- a chain of ~130 small dependent launches each -- run concurrently with
// the trailing update of the previous step on CUs reserved for them (Ctx::lookahead_streams), instead of
// leaving 255 CUs idle.  Same arithmetic per entry as the reference's right-looking sweep
// (cholesky/ldlt/factor.rs:367-498) with a larger step.
// LltPlan: the step table and the knobs; LltPlan::decide: what step k is; LltLookahead: one call, one method per kind of step.
constexpr idx_t LA_NB = 1024;

// Step table of the blocked driver (pure host logic, unit tested without a GPU through faer_hip_debug_llt_plan):
// starts of the look-ahead panels; the last entry is where the sequential tail takes over.  The first step is ONE 128-block,
// the second 512 wide, the following ones nb2 while at least 2 * nb2 rows remain behind them, LA_NB again towards the end;
// steps stop once no more than `tail_rows` rows remain (or the next panel would reach the end of the matrix).
// (the driver runs nb2 = LA_NB: wider later steps -- K = nb2 trailing updates closer to the dense rate, fewer launch
// boundaries -- measured no gain in round 2)
std::vector<idx_t> llt_plan(idx_t n, idx_t tail_rows, idx_t nb2)
{
	// width of the first look-ahead step: the whole chip waits for the first diagonal block, so it is ONE 128-block (a
	// leaf, ~55 us) instead of a 1024-wide one (~1.05 ms): 41.1 -> 40.1 ms at N = 16384
	const idx_t first = POTRF_NB;
	const idx_t second = 512; // (measured: 0 / 256 / 512: 33.54-33.56 / 33.34 / 33.21-33.30 ms at N = 16384)
	std::vector<idx_t> J{0};
	while (true) {
		const idx_t j0 = J.back();
		idx_t w = J.size() == 1 ? LA_NB : nb2;
		if (n - j0 - w < 2 * w)
			w = LA_NB; // narrow steps again towards the end
		if (J.size() == 1 && first < w)
			w = first;
		// the SECOND step: its diagonal chain + panel solve have only the K = `first` update of the whole matrix to hide
		// behind (0.73 ms at N = 16384; a 1024-wide step needs 1.1 + 0.6 ms: the bulk stream idled 1.06 ms)
		if (J.size() == 2 && second < w && n - j0 - second >= 2 * w)
			w = second;
		if (!(n - j0 > tail_rows && j0 + w < n))
			break;
		J.push_back(j0 + w);
	}
	return J;
}

// How P_k, the rows below D_k, gets solved.
enum class LltSolve {
	// Round 4: the panel solve (a dependent chain of ~15 small launches, ~0.4 ms whatever the number of rows: 6.4 of the bulk
	// stream's 34 ms, profiles/r03_llt_timeline.txt) does not sit between two trailing updates on the bulk stream: step k - 1
	// had a plain side stream do it beside the square of its update (LltUpdate::Split), the bulk stream only waits for it.
	OnSide,
	// Round 5: the late steps.  Once the trailing products are shorter than the chains (fewer than side_rmin rows below the
	// next panel) a step was the SUM of two chains: the diagonal block D_{k+1} on the panel stream (24 launches, 0.97 ms), then
	// the solve of all of P_{k+1} on the bulk stream (15 launches, 0.41 ms), then the product of D_{k+2}: 1.48 ms per 1024
	// columns with the trailing product hidden beside the first chain (kernel trace, profiles/r05_exp_llt_driver.txt).  But
	// D_{k+2} needs only the TOP rows X0_{k+1} of P_{k+1} (the next diagonal block's rows), and those can be solved block column
	// by block column right behind the leaves of D_{k+1}: a FOLLOWER on the side stream -- per 128-block one small product and one
	// substitution leaf on w2 rows, behind an event of the leaf that produced the block's packed image -- finishes one block
	// behind the diagonal chain.  The solve of the rows below X0 then runs on the bulk stream BESIDE the next diagonal chain.
	// For the follower to start early the bulk stream brings X0's rows up to date in a launch of their own (and the diagonal
	// block two steps ahead, which shares those rows) before the rest of the product (LltUpdate::BandMerged).
	// Measured (profiles/r05_exp_llt_driver.txt): a late step 1.47 -> 1.36 ms, N = 16384 35.1-35.4 -> 34.9-35.0 ms -- less than the
	// 0.4 ms per step the chains promise: the follower cannot start before the bulk stream has solved the rows that update X0
	// (0.6 ms into the step), its small products run ~5 x slower beside the trailing product, and with the extra launches the
	// bulk stream's own chain (solve 0.41 + four products) is now as long as the panel stream's.
	Follower,
	Bulk // all of it on the bulk stream behind D_k: the last step, when nothing was solved ahead
};
// How step k updates the trailing matrix.  Every kind but Last stands for one LltSolve of step k + 1 (LltPlan::decide).
enum class LltUpdate {
	Last,	    // one product on the whole trailing matrix; the tail driver takes over
	Merged,	    // block column k + 1 below D_{k+1} + the lower square right of it in ONE launch (tri_skip)        -> Bulk
	BandMerged, // the rows of X0_{k+1} and of D_{k+2} first (ONE band launch), then the merged product below them;
		    // D_{k+1} is factored with a follower                                                            -> Follower
	// Block column k + 1 FIRST (its own launch), and while the lower square right of it -- which neither reads nor writes
	// that block column -- runs on the bulk stream, the side stream solves P_{k+1} = A_{>k+1,k+1} L_{k+1,k+1}^-T as soon as the
	// panel stream has factored the diagonal block.  Its small kernels find their slots among the product's workgroups (the
	// two launches are independent); it pays only while the square is much longer than the chain it hides.       -> OnSide
	Split
};
// Where A_{k+1,k+1} -= X0 X0^T runs, X0 = the top rows of P_k.  (None <=> Last, WithFollower <=> LltSolve::Follower of the same
// step: a follower step is never the last one, arrival() asks for k + 1 < nsteps.)
enum class LltNextDiag {
	None,	      // the last step has no next diagonal block
	WithFollower, // on the bulk stream as soon as the follower has X0, before the rows below X0 are solved
	OnPanel,      // on the panel stream: it has slack to spare while the trailing matrix is large, the bulk stream issues fewer launches
	BulkFirst     // first launch of the update on the bulk stream
};

struct LltStep {
	idx_t j0, j1, w, r; // panel columns [j0, j1), w of them; r rows below
	idx_t w1, w2;	    // widths of the next two look-ahead panels (0: there is none)
	LltSolve solve;
	LltUpdate update;
	LltNextDiag diag;
	bool follower_next() const { return update == LltUpdate::BandMerged; } // D_{k+1} is factored with a follower
};

// The schedule of one blocked factorization: pure host data.  The knobs are read here and nowhere else (FAER_HIP_LLT_*: the
// tests lower them to reach every kind of step at small sizes).
// Once the remaining matrix is small the chain "diagonal block -> panel solve -> next diagonal block" is longer than the
// trailing update it is meant to hide behind: below la_min and for the last tail_rows rows of a large matrix the steps run
// back to back on the caller's stream (potrf_blocked).  Look-ahead pays from ~10k rows upwards (measured, N = 8192: 13.3 ms
// sequential against 13.8 ms); round 5, right-looking diagonal chains: look-ahead from 8192 rows on -- 9.5 ms either way there,
// 6144: 6.2 sequential against 6.5 -- and down to the last 1024 rows: tails of 4096 / 3072 / 2048 / 1024 rows 34.1 / 33.6-33.7 /
// 33.4 / 33.2 ms at N = 16384.  side_rmin / dpanel_rmin re-swept with the right-looking chains: side solve from 4096 / 6144 / 8192 /
// 10240 rows 33.7 / 33.0-33.2 / 33.1-33.6 / 33.6-34.0 ms, next diagonal block's product on the panel stream from 4096 / 8192 / 12288
// rows 33.2 / 33.1-33.6 / 33.6-33.9: both left at 8192.
struct LltPlan {
	idx_t n, la_min, tail_rows; // smallest n on the blocked path; rows left to the sequential tail
	idx_t side_rmin;	    // rows below a panel from which the side stream solves it
	idx_t dpanel_rmin;	    // rows below panel k from which the update of D_{k+1} runs on the panel stream
	std::vector<idx_t> J{0};    // look-ahead step k factors the columns [J[k], J[k + 1]); the tail starts at J.back()
	LltPlan(idx_t n, idx_t la_min, idx_t tail_rows, idx_t side_rmin, idx_t dpanel_rmin)
		: n(n), la_min(la_min), tail_rows(tail_rows), side_rmin(side_rmin), dpanel_rmin(dpanel_rmin)
	{
		if (blocked())
			J = llt_plan(n, tail_rows, LA_NB);
	}
	static idx_t knob(const char *name, idx_t dflt) { return getenv(name) ? (idx_t) atol(getenv(name)) : dflt; }
	explicit LltPlan(idx_t n)
		: LltPlan(n, knob("FAER_HIP_LLT_LA_MIN", 2 * LA_NB), knob("FAER_HIP_LLT_TAIL", n < 8 * LA_NB ? n : LA_NB),
			  knob("FAER_HIP_LLT_SIDE_RMIN", 8192), knob("FAER_HIP_LLT_DPANEL_RMIN", 8192)) {}
	bool blocked() const { return n >= la_min && n > LA_NB; }
	idx_t nsteps() const { return (idx_t) J.size() - 1; }
	LltSolve arrival(idx_t k) const
	{
		if (k >= 1 && n - J[(size_t) k + 1] >= side_rmin)
			return LltSolve::OnSide;
		return k + 1 < nsteps() ? LltSolve::Follower : LltSolve::Bulk;
	}
	LltStep decide(idx_t k) const
	{
		const idx_t j0 = J[(size_t) k], j1 = J[(size_t) k + 1];
		LltStep s{j0, j1, j1 - j0, n - j1, 0, 0, arrival(k), LltUpdate::Last, LltNextDiag::None};
		if (k + 1 == nsteps())
			return s;
		s.w1 = J[(size_t) k + 2] - j1;
		const LltSolve next = arrival(k + 1);
		s.update = next == LltSolve::OnSide ? LltUpdate::Split : next == LltSolve::Follower ? LltUpdate::BandMerged : LltUpdate::Merged;
		if (next == LltSolve::Follower) // (then k + 2 < nsteps: J[k + 3] exists)
			s.w2 = J[(size_t) k + 3] - J[(size_t) k + 2];
		s.diag = s.solve == LltSolve::Follower ? LltNextDiag::WithFollower : s.r >= dpanel_rmin ? LltNextDiag::OnPanel : LltNextDiag::BulkFirst;
		return s;
	}
};
// faer_hip_debug_llt_steps: the decisions of every look-ahead step as integers (the enums' values); the streams are assumed
size_t llt_debug_steps(idx_t n, idx_t la_min, idx_t tail_rows, idx_t side_rmin, idx_t dpanel_rmin, int *codes, size_t cap)
{
	const LltPlan p(n, la_min, tail_rows, side_rmin, dpanel_rmin);
	for (idx_t k = 0; k < p.nsteps() && (size_t) k < cap; ++k) {
		const LltStep s = p.decide(k);
		const int row[4] = {(int) s.solve, (int) s.update, (int) s.diag, (int) s.follower_next()};
		std::copy(row, row + 4, codes + 4 * k);
	}
	return (size_t) p.nsteps();
}

template <typename T> struct LltLookahead {
	MatV<T> A;
	const CholWork<T> &wk;
	const LltPlan &plan;
	hipStream_t caller;
	Ctx &c = ctx();
	hipStream_t side = nullptr;
	// across steps (what it says: who records it -> who waits for it):
	hipEvent_t ev_diag = nullptr; // D_k is factored, its packed blocks are in wk: factor_diag, panel stream -> solve_bulk; side_solve of step k - 1
	hipEvent_t ev_x0 = nullptr;   // X0_k is solved by the follower (implies ev_diag): factor_diag, side stream -> solve_follower
	hipEvent_t ev_side = nullptr; // P_k is solved: side_solve of step k - 1 -> the bulk stream of step k (LltSolve::OnSide)
	// inside a step, recorded on the bulk stream:
	hipEvent_t ev_solved = nullptr; // P_k is solved -> the panel stream where it updates D_{k+1} itself (OnPanel)
	hipEvent_t ev_col = nullptr;	// D_{k+1} is up to date (Split: all of block column k + 1) -> the panel stream otherwise; side_solve
	hipEvent_t ev_band = nullptr;	// the rows of X0_{k+1} are up to date (BandMerged) -> the follower of D_{k+1}
	hipEvent_t record(hipStream_t s)
	{
		hipEvent_t e = c.next_event();
		FH_HIP(hipEventRecord(e, s));
		return e;
	}
	MatV<T> panel(const LltStep &s) const { return A.sub(s.j1, s.j0, s.r, s.w); }		 // P_k
	MatV<T> below_x0(const LltStep &s) const { return A.sub(s.j1 + s.w1, s.j0, s.r - s.w1, s.w); } // P_k without X0
	MatV<const T> diag_block(const LltStep &s) const { return A.sub(s.j0, s.j0, s.w, s.w).c(); }
	// D_k on the current (panel) stream, with the follower for X0_k if that panel is solved that way; the follower must not start
	// before `rows_ready`: the rows of X0_k are up to date with panel k - 1 (null for the first panel)
	void factor_diag(idx_t k, bool follower, hipEvent_t rows_ready)
	{
		const idx_t j0 = plan.J[(size_t) k], j1 = plan.J[(size_t) k + 1], w = j1 - j0;
		MatV<T> D = A.sub(j0, j0, w, w);
		if (!follower) {
			potrf_panel_flat<T>(D, wk, j0);
		} else {
			MatV<T> X0 = A.sub(j1, j0, plan.J[(size_t) k + 2] - j1, w);
			if (rows_ready)
				stream_wait(side, rows_ready);
			potrf_panel_flat_hook<T>(D, wk, j0, [&](idx_t c0, idx_t nb, T *W) {
				hipEvent_t leaf = record(c.la_panel);
				StreamScope ss(side);
				stream_wait(side, leaf);
				follow_block(D, X0, c0, nb, W);
			});
			ev_x0 = record(side);
		}
		ev_diag = record(c.la_panel);
	}
	// the follower behind the leaf of block column c0 of D.  RIGHT-looking on the rows of X0: solve block column c0, then take it
	// out of the block columns right of it (K = 128 products: ~15 us each; the left-looking form with K = c0 on w1 x 128 outputs
	// took ~100 us per block and the follower finished 0.34 ms behind the diagonal chain -- kernel trace r5v29)
	void follow_block(MatV<T> D, MatV<T> X0, idx_t c0, idx_t nb, const T *W)
	{
		const idx_t w = D.ncols, w1 = X0.nrows, c1 = c0 + nb;
		trsm_lower_pre_dev<T>(D.sub(c0, c0, nb, nb).c(), X0.sub(0, c0, w1, nb).t(), W);
		if (c1 < w)
			gemm_dev<T>(X0.sub(0, c1, w1, w - c1), DST_FULL, true, X0.sub(0, c0, w1, nb).c(), D.sub(c1, c0, w - c1, nb).t().c(), (T) -1);
	}
	// A_{k+1,k+1} -= X0 X0^T on the current stream
	void update_next_diag(const LltStep &s)
	{
		MatV<const T> X0 = panel(s).sub(0, 0, s.w1, s.w).c();
		gemm_dev<T>(A.sub(s.j1, s.j1, s.w1, s.w1), DST_LOWER, true, X0, X0.t(), (T) -1);
	}

	// X0_k came from the follower: the next diagonal block at once (-> the panel stream), then the rows below X0_k
	void solve_follower(const LltStep &s)
	{
		stream_wait(c.la_bulk, ev_x0);
		update_next_diag(s);
		ev_col = record(c.la_bulk);
		if (s.r > s.w1)
			trsm_lower_pre_dev<T>(diag_block(s), below_x0(s).t(), wk.wslot(s.j0));
	}
	// P_k <- P_k L_kk^-T in place (cholesky/ldlt/factor.rs:422-426): the reference's TRSM recursion on the 128-blocks of
	// L_kk -- substitution leaves against the packed diagonal blocks the panel stream left in wk, MFMA products in between
	void solve_bulk(const LltStep &s)
	{
		stream_wait(c.la_bulk, ev_diag);
		trsm_lower_pre_dev<T>(diag_block(s), panel(s).t(), wk.wslot(s.j0));
	}

	// the trailing matrix, one method per LltUpdate
	void update_last(const LltStep &s)
	{
		MatV<const T> X = panel(s).c();
		gemm_dev<T>(A.sub(s.j1, s.j1, s.r, s.r), DST_LOWER, true, X, X.t(), (T) -1);
	}
	void update_merged(const LltStep &s)
	{
		if (s.diag == LltNextDiag::BulkFirst) {
			update_next_diag(s);
			ev_col = record(c.la_bulk);
		}
		GemmExtra<T> ex;
		ex.tri_skip = s.w1;
		if (s.update == LltUpdate::BandMerged) {
			// the rows of X0_{k+1} (the follower of the next diagonal block waits for them) and, in the same rows, the
			// diagonal block two steps ahead; the merged product below then skips these rows as well
			// (ONE launch: the rows [w1, w1 + w2) of the lower triangle of the leading (w1 + w2)^2 block)
			const idx_t wb = s.w1 + s.w2;
			MatV<const T> X01 = panel(s).sub(0, 0, wb, s.w).c();
			gemm_dev<T>(A.sub(s.j1, s.j1, wb, wb), DST_LOWER, true, X01, X01.t(), (T) -1, &ex);
			ev_band = record(c.la_bulk);
			ex.tri_skip = wb;
		}
		// block column k + 1 below its diagonal block + the remaining lower square in ONE launch: the lower triangle of the
		// whole trailing matrix minus its leading rows
		MatV<const T> X = panel(s).c();
		if (ex.tri_skip < s.r)
			gemm_dev<T>(A.sub(s.j1, s.j1, s.r, s.r), DST_LOWER, true, X, X.t(), (T) -1, &ex);
	}
	void update_split(const LltStep &s)
	{
		if (s.diag == LltNextDiag::BulkFirst)
			update_next_diag(s);
		const idx_t jc = s.j1 + s.w1, rc = s.r - s.w1;
		MatV<const T> X2 = below_x0(s).c();
		// block column k + 1 below its diagonal block
		gemm_dev<T>(A.sub(jc, s.j1, rc, s.w1), DST_FULL, true, X2, panel(s).sub(0, 0, s.w1, s.w).c().t(), (T) -1);
		ev_col = record(c.la_bulk);
		// the remaining lower square
		gemm_dev<T>(A.sub(jc, jc, rc, rc), DST_LOWER, true, X2, X2.t(), (T) -1);
	}
	// P_{k+1} on the side stream beside the square of update_split
	void side_solve(const LltStep &s)
	{
		StreamScope sc(side);
		stream_wait(side, ev_col);
		stream_wait(side, ev_diag);
		trsm_lower_pre_dev<T>(A.sub(s.j1, s.j1, s.w1, s.w1).c(), A.sub(s.j1 + s.w1, s.j1, s.r - s.w1, s.w1).t(), wk.wslot(s.j1));
		ev_side = record(side);
	}

	void run()
	{
		c.reset_events();
		hipEvent_t e0 = record(caller);
		stream_wait(c.la_bulk, e0);
		stream_wait(c.la_panel, e0);
		c.qr_side_streams();
		side = c.qr_side[0];
		{
			StreamScope sc(c.la_panel);
			factor_diag(0, plan.arrival(0) == LltSolve::Follower, nullptr);
		}
		for (idx_t k = 0; k < plan.nsteps(); ++k) {
			const LltStep s = plan.decide(k);
			{
				StreamScope sc(c.la_bulk);
				if (s.solve == LltSolve::OnSide)
					stream_wait(c.la_bulk, ev_side);
				else if (s.solve == LltSolve::Follower)
					solve_follower(s);
				else
					solve_bulk(s);
				ev_solved = record(c.la_bulk);
				if (s.update == LltUpdate::Last)
					update_last(s);
				else if (s.update == LltUpdate::Split)
					update_split(s);
				else
					update_merged(s);
			}
			if (s.update == LltUpdate::Last) // (it starts nothing on the panel or the side stream)
				break;
			{
				StreamScope sc(c.la_panel);
				stream_wait(c.la_panel, s.diag == LltNextDiag::OnPanel ? ev_solved : ev_col);
				if (s.diag == LltNextDiag::OnPanel)
					update_next_diag(s);
				// (the follower of D_{k+1} must not start before X0_{k+1}'s rows are up to date with panel k: ev_band says so)
				factor_diag(k + 1, s.follower_next(), s.follower_next() ? ev_band : nullptr);
			}
			if (s.update == LltUpdate::Split)
				side_solve(s);
		}
		// rejoin the caller's stream (the side stream's last launch was waited for by the bulk stream)
		hipEvent_t eb = record(c.la_bulk), ep = record(c.la_panel);
		stream_wait(caller, eb);
		stream_wait(caller, ep);
	}
};

// The blocked driver: the look-ahead steps of the plan, then the tail (everything, if there are no steps) -- sequential, whole
// chip, on the caller's stream: one tall panel (potrf_panel_flat) + ONE trailing update per step.
// (steps of 128 / 256 / 512 / 2048 columns here: 34.2-34.3 / 34.3 / 34.4-34.5 ms at N = 16384 against 34.0-34.1; N = 8192: 10.4 / 9.7 / 9.6 / 9.8 against 9.65)
template <typename T> static void potrf_blocked(MatV<T> A, const CholWork<T> &wk, LltPlan plan)
{
	const idx_t n = A.nrows;
	if (plan.nsteps() > 0 && !ctx().lookahead_streams())
		plan.J.resize(1); // (without the look-ahead streams everything is the tail)
	if (plan.nsteps() > 0)
		LltLookahead<T>{A, wk, plan, ctx().stream}.run();
	for (idx_t j0 = plan.J.back(); j0 < n; j0 += LA_NB) {
		const idx_t w = LA_NB < n - j0 ? LA_NB : n - j0, R = n - j0;
		potrf_panel_flat<T>(A.sub(j0, j0, R, w), wk, j0);
		if (R > w) {
			MatV<const T> P2 = A.sub(j0 + w, j0, R - w, w).c();
			gemm_dev<T>(A.sub(j0 + w, j0 + w, R - w, R - w), DST_LOWER, true, P2, P2.t(), (T) -1);
		}
	}
}

// Tall panel entry point for the distributed driver (dist_llt.h): Cholesky of the top square block of P and the
// solve of the rows below it, right-looking in 128-column blocks (potrf_panel_flat).  status: 2 device ints,
// [0] = first failing global index + 1 (kept if already set), [1] += regularisation count; no synchronisation.
template <typename T> void potrf_panel_dev(MatV<T> P, T reg_delta, T reg_eps, int *status_dev, idx_t offset)
{
	FH_CHECK(P.nrows >= P.ncols, "potrf_panel: the panel must be tall");
	if (P.ncols == 0)
		return;
	const idx_t nblk = (P.ncols + POTRF_NB - 1) / POTRF_NB;
	Scratch winv((size_t) nblk * TriPack<T>::BYTES);
	const int regularize = (reg_delta > (T) 0 && reg_eps > (T) 0) ? 1 : 0;
	potrf_panel_flat<T>(P, CholWork<T>{regularize, reg_eps, reg_delta, status_dev, winv.as<T>(), offset / POTRF_NB}, offset);
}
template void potrf_panel_dev<double>(MatV<double>, double, double, int *, idx_t);
template void potrf_panel_dev<float>(MatV<float>, float, float, int *, idx_t);

// What a whole factorization (LLT or LDLT) sets up and reads back: the zeroed status word, one packed image per diagonal block (only
// those some TRSM will use are filled), the regularisation rule (cholesky/llt/factor.rs:85-86, cholesky/ldlt/factor.rs:766-767)
template <typename T> struct CholCall {
	Scratch st{64}, winv;
	CholWork<T> wk;
	CholCall(idx_t n, T reg_delta, T reg_eps)
		: winv(n > POTRF_NB ? (size_t) ((n + POTRF_NB - 1) / POTRF_NB) * TriPack<T>::BYTES : 256),
		  wk{(reg_delta > (T) 0 && reg_eps > (T) 0) ? 1 : 0, reg_eps, reg_delta, st.as<int>(), winv.as<T>()}
	{
		FH_HIP(hipMemsetAsync(wk.status, 0, 64, ctx().stream));
	}
	// the one synchronisation of the call; >= 0: regularisation count, < 0: -(index + 1) of the failing pivot
	long finish()
	{
		int h[2] = {0, 0};
		FH_HIP(hipMemcpyAsync(h, wk.status, sizeof(h), hipMemcpyDeviceToHost, ctx().stream));
		ctx().sync();
		ctx().quiesce();
		return h[0] != 0 ? -(long) h[0] : (long) h[1];
	}
};

template <typename T> long potrf_lower_dev(MatV<T> A, T reg_delta, T reg_eps)
{
	FH_CHECK(A.nrows == A.ncols, "potrf: matrix must be square");
	FH_CHECK(A.nrows < (1L << 30), "potrf: matrix too large");
	if (A.nrows == 0)
		return 0;
	CholCall<T> call(A.nrows, reg_delta, reg_eps);
	const LltPlan plan(A.nrows);
	if (plan.blocked())
		potrf_blocked<T>(A, call.wk, plan);
	else
		chol_rec<T, false>(A, call.wk, 0, false);
	const long ret = call.finish();
#ifdef FH_LEAF_TIMING
	{
		unsigned long long d[8];
		FH_HIP(hipMemcpyFromSymbol(d, HIP_SYMBOL(g_leaf_timing), sizeof(d)));
		fprintf(stderr, "leaf timing (cycles, thread 0, cumulative): load %llu | panel %llu | syrk %llu | store %llu | inverse %llu | store W %llu\n",
			d[0], d[1], d[2], d[3], d[4], d[5]);
	}
#endif
	return ret;
}

// L D L^T (chol_rec<T, true>).  `signs_host`: n int8 or NULL.
template <typename T> long sytrf_lower_dev(MatV<T> A, T reg_delta, T reg_eps, const signed char *signs_host)
{
	FH_CHECK(A.nrows == A.ncols, "ldlt: matrix must be square");
	FH_CHECK(A.nrows < (1L << 30), "ldlt: matrix too large");
	if (A.nrows == 0)
		return 0;
	const idx_t n = A.nrows;
	CholCall<T> call(n, reg_delta, reg_eps);
	Scratch dv((size_t) n * sizeof(T)), sg((size_t) n + 256);
	call.wk.Dv = dv.as<T>();
	if (signs_host && call.wk.regularize) {
		FH_HIP(hipMemcpyAsync(sg.p, signs_host, (size_t) n, hipMemcpyHostToDevice, ctx().stream));
		call.wk.signs = sg.as<signed char>();
	}
	chol_rec<T, true>(A, call.wk, 0, false);
	return call.finish();
}

template long sytrf_lower_dev<double>(MatV<double>, double, double, const signed char *);
template long sytrf_lower_dev<float>(MatV<float>, float, float, const signed char *);
template long potrf_lower_dev<double>(MatV<double>, double, double);
template long potrf_lower_dev<float>(MatV<float>, float, float);

} // namespace fh
