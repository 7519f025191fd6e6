// Householder QR without pivoting for gfx950.
//
// Replaces faer/src/linalg/qr/no_pivoting/factor.rs:11-301 and the pieces of
// faer/src/linalg/householder.rs it uses (make_householder_imp :59-107, upgrade_householder_factor :132-272,
// apply_block_householder_* :370-808) -- SURVEY.md section 8a rows a24-a30.
//
// Output convention (householder.rs:1-33): R in the upper triangle, the tails of the reflectors v_j
// (v_jj = 1 implicit) below it, and Q_coeff = one upper triangular T per block of `block_size` columns
// with T_jj = tau_j = |v_j|^2 / 2 and T_ij = v_i^H v_j (i < j), so that H_0 .. H_{b-1} = I - V T^-1 V^H.
//
// Two paths, both on the GPU:
//  * FAST (full column rank, the case of every benchmark shape): the reference's recursion on the block
//    size (factor.rs:137-256), with every level-3 step on the MFMA GEMM (split-K for the K = nrows inner
//    products) and an 8-column cooperative leaf: the panel's row chunks stay resident in LDS across the 8
//    column steps, each step needs ONE device-wide reduction (the dot products x^H a_c of the current column
//    with all remaining panel columns are summed in the same pass that would compute its norm, so the
//    reflector, its tau and the update all follow from one all-reduce), plus one more for the 8x8 T block.
//    The rank test of the reference (factor.rs:52-82) is evaluated on the fly; the first column that fails
//    it raises a flag and the factorization is redone from a saved copy by
//  * GENERAL (rank revealing): a literal restatement of qr_in_place_unblocked (factor.rs:11-86) with the
//    running `row` kept in device memory (no host round trip per column), followed by the T blocks
//    T = striu(V^H V) + diag(tau) per block of accepted reflectors.
#include <atomic>
#include <climits>
#include <limits>

#include "common.h"
#include "reduce.h"
#include "xwg.h"

namespace fh {

// ------------------------------------------------------------------------------------------------
// block reflector application (householder.rs:370-620, generic path)
// ------------------------------------------------------------------------------------------------
// M <- (I - V T^-H V^H) M  (forward)   or   (I - V T^-1 V^H) M  (!forward); V unit lower trapezoidal m x b
template <typename T> static void apply_block_householder_dev(MatV<const T> V, MatV<const T> Tf, MatV<T> M, bool forward)
{
	const idx_t m = V.nrows, b = V.ncols, k = M.ncols;
	if (b == 0 || k == 0 || m == 0)
		return;
	FH_CHECK(Tf.nrows == b && Tf.ncols == b && M.nrows == m && m >= b, "apply_block_householder: shape mismatch");
	Scratch tmpb((size_t) b * (size_t) k * sizeof(T));
	MatV<T> tmp{tmpb.as<T>(), b, k, 1, b};
	MatV<const T> Vtop = V.sub(0, 0, b, b), Vbot = V.sub(b, 0, m - b, b);
	MatV<T> Mtop = M.sub(0, 0, b, k), Mbot = M.sub(b, 0, m - b, k);
	// tmp = V_top^H M_top + V_bot^H M_bot   (householder.rs:541-563)
	matmul_triangular_dev<T>(tmp, 0, false, Vtop.t(), 6 /*unit upper*/, Mtop.c(), 0, (T) 1);
	if (m > b) {
		GemmExtra<T> big;
		big.prefer_big_tiles = true;
		gemm_dev<T>(tmp, DST_FULL, true, Vbot.t(), Mbot.c(), (T) 1, &big);
	}
	// tmp <- T^-H tmp or T^-1 tmp          (householder.rs:564-578)
	if (forward)
		trsm_lower_dev<T>(Tf.t(), false, tmp);
	else
		trsm_upper_dev<T>(Tf, false, tmp);
	// M -= V tmp                            (householder.rs:579-601)
	matmul_triangular_dev<T>(Mtop, 0, true, Vtop, 5 /*unit lower*/, tmp.c(), 0, (T) -1);
	if (m > b)
		gemm_dev<T>(Mbot, DST_FULL, true, Vbot, tmp.c(), (T) -1);
}

// householder.rs:724-808
template <typename T>
void apply_householder_sequence_left_dev(MatV<const T> V, MatV<const T> H, MatV<T> M, bool transpose)
{
	const idx_t m = V.nrows, n = V.ncols;
	const idx_t size = m < n ? m : n;
	const idx_t block_size = H.nrows;
	FH_CHECK(block_size > 0 && H.ncols == size && M.nrows == m, "apply_householder_sequence: shape mismatch");
	if (transpose) {
		for (idx_t j = 0; j < size;) {
			const idx_t bs = block_size < size - j ? block_size : size - j;
			apply_block_householder_dev<T>(V.sub(j, j, m - j, bs), H.sub(0, j, bs, bs), M.sub(j, 0, m - j, M.ncols),
						       true);
			j += bs;
		}
	} else {
		idx_t j = size;
		idx_t bs = size % block_size;
		if (bs == 0)
			bs = block_size;
		while (j > 0) {
			const idx_t jp = j - bs;
			bs = block_size;
			apply_block_householder_dev<T>(V.sub(jp, jp, m - jp, j - jp), H.sub(0, jp, j - jp, j - jp),
						       M.sub(jp, 0, m - jp, M.ncols), false);
			j = jp;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// FAST path leaf: cooperative 8-column Householder panel
// ------------------------------------------------------------------------------------------------
constexpr int QR_PW = 8;
constexpr int QR_GMAX = 512;
constexpr int QR_NPAIR = QR_PW * (QR_PW - 1) / 2; // 28
constexpr int QR_SLOT = 32;			  // doubles per workgroup slot (>= QR_NPAIR, >= QR_PW)

template <typename T> struct QrPanelArgs {
	T *P;	     // panel view, row 0 = diagonal row of its first column
	idx_t rs, cs;
	int m, w;
	int R;
	const T *above; // A[0, abs_col0] (rows above the panel), same strides
	int row_abs;	// number of rows above the panel
	T *Tb;		// w x w block of Q_coeff (upper)
	idx_t trs, tcs;
	double *slots; // [2][G][QR_SLOT]
	double *head;  // [2][QR_PW + 1]: row j of the panel (cols j..w) and |above|^2
	xwg_u64 *flags; // [G] per-workgroup epoch flags (xwg.h)
	xwg_u64 *gran;	// [2][G][2 * QR_PW] tagged granules: the QR_PW column sums of every workgroup (column steps)
	xwg_u64 *gran_head; // [2][2 * (QR_PW + 1)]: row j of the panel and |above|^2, published by workgroup 0
	xwg_u64 epoch_base;
	int *status; // [2] exchange timeout, [3] rank deficiency detected
};

// ------------------------------------------------------------------------------------------------
// Register-resident panel kernel: every thread keeps QR2_RPT whole panel rows (8 columns each) in registers and
// the 8 column steps are unrolled at compile time, so the dot products x^H a_c, the scaling and the rank-1 update
// are register FMAs (in the first, LDS-resident version of this kernel the LDS loops were ~3/4 of its time,
// exactly as in the LU panel: profiles/r01_lu_panel_phase_timing.txt).
// ------------------------------------------------------------------------------------------------
constexpr int QR2_NT = 512;
template <typename T> static constexpr int qr2_rpt() { return sizeof(T) == 8 ? 4 : 8; }

template <typename T> struct Qr2Shared {
	double part[(QR2_NT / 64) * QR_SLOT], red[QR_SLOT], S[QR_SLOT];
	double tau[QR_PW], head[QR_PW + 1];
	T top[QR_PW][QR_PW]; // rows 0..7 of the panel (chunk 0): top[r][c]
	int flag;
};

// one column step; false: leave (timeout or rank deficiency recorded in `why`)
template <typename T, int RPT, int J>
static __device__ __forceinline__ bool qr2_step(const QrPanelArgs<T> &a, T (&x)[RPT][QR_PW], Qr2Shared<T> &sh, int r0, int G, int &bar,
						int &why)
{
	const int tid = threadIdx.x;
	const int g = blockIdx.x;
	const int w = a.w;
	const int q = bar & 1;
	// ---- partial sums s_c = sum_{r > J} x_r a_rc, c = J .. w-1 (c == J gives |tail|^2)
	double acc[QR_PW];
#pragma unroll
	for (int c = 0; c < QR_PW; ++c)
		acc[c] = 0.0;
	double ab[1] = {0.0};
#pragma unroll
	for (int i = 0; i < RPT; ++i) {
		const int gr = r0 + tid + i * QR2_NT;
		if (gr > J && gr < a.m) {
			const double xv = (double) x[i][J];
#pragma unroll
			for (int c = J; c < QR_PW; ++c)
				if (c < w)
					acc[c] += xv * (double) x[i][c];
		}
		if (gr < J) { // rows of the panel above the diagonal (chunk 0 only): part of |above|^2
			const double v = (double) x[i][J];
			ab[0] += v * v;
		}
	}
	block_sum<QR2_NT, QR_PW>(acc, sh.part, sh.red);
	// row J of the panel lives in thread J of chunk 0
	if (g == 0 && tid == J) {
#pragma unroll
		for (int c = 0; c < QR_PW; ++c)
			sh.top[J][c] = x[0][c];
	}
	if (g == 0) {
		// rows above the panel (outside it)
		for (int i = tid; i < a.row_abs; i += QR2_NT) {
			const double v = (double) a.above[(idx_t) i * a.rs + (idx_t) J * a.cs];
			ab[0] += v * v;
		}
		block_sum<QR2_NT, 1>(ab, sh.part, sh.S); // sh.S[0] = |above|^2 (also publishes sh.top through its barriers)
	}
	if (G > 1) {
		// All-reduce of the QR_PW column sums with data-tagged granules (xwg.h, recipe R2): {tag, 32 payload bits}
		// per 8-byte write-through store, no store drain, no flag, and the consumers fetch sums AND row j in the
		// same round: one store latency + one load latency per column instead of drain + flag + two dependent
		// reads.  Every thread owns the pairs pe = tid + QR2_NT * i of the G x QR_PW table, i.e. always column
		// c = tid % QR_PW: fixed summation order (i ascending, lanes by xor 8 / 16 / 32, waves ascending).
		const unsigned tag = (unsigned) (a.epoch_base + (xwg_u64) (bar + 1));
		if (tid < QR_PW || (g == 0 && tid <= 2 * QR_PW)) {
			const double v = tid < QR_PW ? sh.red[tid] : tid < 2 * QR_PW ? (tid - QR_PW < w ? (double) sh.top[J][tid - QR_PW] : 0.0) : sh.S[0];
			xwg_u64 *dst = tid < QR_PW ? a.gran + ((size_t) q * G + g) * (2 * QR_PW) + 2 * tid
					       : a.gran_head + (size_t) q * 2 * (QR_PW + 1) + 2 * (tid - QR_PW);
			const xwg_u64 vb = (xwg_u64) __double_as_longlong(v);
			xwg_store_gran(dst, tag, (unsigned) (vb >> 32));
			xwg_store_gran(dst + 1, tag, (unsigned) vb);
		}
		constexpr int MAXI = QR_GMAX * QR_PW / QR2_NT;
		const int np = G * QR_PW;
		xwg_u64 hi[MAXI], lo[MAXI], hh = 0, hl = 0;
		const xwg_u64 *gq = a.gran + (size_t) q * G * (2 * QR_PW);
		const xwg_u64 *hq = a.gran_head + (size_t) q * 2 * (QR_PW + 1) + 2 * (tid <= QR_PW ? tid : 0);
		int ok = 0;
		for (int spin = 0; spin < (1 << 21); ++spin) {
			bool all = true;
#pragma unroll
			for (int i = 0; i < MAXI; ++i) {
				const int pe = tid + QR2_NT * i;
				if (pe < np) {
					hi[i] = xwg_load_gran(gq + 2 * pe);
					lo[i] = xwg_load_gran(gq + 2 * pe + 1);
					all = all && (unsigned) (hi[i] >> 32) == tag && (unsigned) (lo[i] >> 32) == tag;
				}
			}
			if (tid <= QR_PW) {
				hh = xwg_load_gran(hq);
				hl = xwg_load_gran(hq + 1);
				all = all && (unsigned) (hh >> 32) == tag && (unsigned) (hl >> 32) == tag;
			}
			if (__all(all)) {
				ok = 1;
				break;
			}
			__builtin_amdgcn_s_sleep(1);
		}
		if (!__syncthreads_and(ok)) {
			why = 2;
			return false;
		}
		++bar;
		double mine = 0.0;
#pragma unroll
		for (int i = 0; i < MAXI; ++i)
			if (tid + QR2_NT * i < np)
				mine += __longlong_as_double((long long) (((hi[i] & 0xffffffffull) << 32) | (lo[i] & 0xffffffffull)));
		mine += __shfl_xor(mine, 8, 64);
		mine += __shfl_xor(mine, 16, 64);
		mine += __shfl_xor(mine, 32, 64);
		if ((tid & 63) < QR_PW)
			sh.part[(tid >> 6) * QR_PW + (tid & 63)] = mine;
		__syncthreads();
		if (tid < QR_PW) {
			double t = 0.0;
#pragma unroll
			for (int k = 0; k < QR2_NT / 64; ++k)
				t += sh.part[k * QR_PW + tid];
			sh.S[tid] = t;
		}
		if (tid <= QR_PW)
			sh.head[tid] = __longlong_as_double((long long) (((hh & 0xffffffffull) << 32) | (hl & 0xffffffffull)));
	} else {
		__syncthreads(); // sh.S[0] (|above|^2) read below before sh.S is overwritten
		const double above2 = sh.S[0];
		__syncthreads();
		if (tid < QR_PW) {
			sh.S[tid] = sh.red[tid];
			sh.head[tid] = tid < w ? (double) sh.top[J][tid] : 0.0;
		}
		if (tid == 0)
			sh.head[QR_PW] = above2;
	}
	__syncthreads();
	// ---- reflector (householder.rs:59-107), evaluated identically by every thread
	T head = (T) sh.head[J];
	const double above2 = sh.head[QR_PW];
	const T tail_norm = (T) sqrt(sh.S[J]);
	T head_norm = fabs(head);
	if (head_norm < Lim<T>::minpos) {
		head = (T) 0;
		head_norm = (T) 0;
	}
	if (tail_norm < Lim<T>::minpos) {
		// householder.rs:70-77 + factor.rs:59-63: tau = inf, nothing is scaled or updated; the column
		// is accepted iff its head is non zero (e.g. the last column of a square matrix)
		if (!(head_norm > (T) 0)) {
			why = 3;
			return false;
		}
		if (tid == 0)
			sh.tau[J] = (double) std::numeric_limits<T>::infinity();
		__syncthreads();
		return true;
	}
	const T norm = (T) hypot((double) head_norm, (double) tail_norm);
	const T sign = head_norm != (T) 0 ? head * ((T) 1 / head_norm) : (T) 1;
	const T signed_norm = sign * norm;
	const T hinv = (T) 1 / (head + signed_norm);
	const T tn = tail_norm * fabs(hinv);
	const T tau = (T) 0.5 * ((T) 1 + tn * tn);
	// rank test (factor.rs:52-82)
	const T full_norm = (T) hypot((double) norm, sqrt(above2));
	const T threshold = Lim<T>::eps * (T) ((double) (a.m - J) * 16.0) * full_norm;
	const T tau_inv = (T) 1 / tau;
	if (tau_inv < Lim<T>::minpos || !(norm > threshold)) {
		why = 3;
		return false;
	}
	if (tid == 0)
		sh.tau[J] = (double) tau;
	// ---- update: v = x * hinv ; k_c = -(a_jc + v^H a_c) / tau ; a_c += k_c v   (factor.rs:65-80)
	T kc[QR_PW];
#pragma unroll
	for (int c = 0; c < QR_PW; ++c)
		// (sh.S[c] = x_J^H a_c carries the SQUARE of the data's scale: outside the range of fp32 for entries beyond 2^+-63 although
		// v^H a_c = hinv * S[c] is not -- the product is formed in fp64 before it is rounded to T; unchanged for T = double)
		kc[c] = (c > J && c < w) ? -(((T) sh.head[c] + (T) ((double) hinv * sh.S[c])) * tau_inv) : (T) 0;
#pragma unroll
	for (int i = 0; i < RPT; ++i) {
		const int gr = r0 + tid + i * QR2_NT;
		if (gr > J && gr < a.m) {
			const T v = x[i][J] * hinv;
			x[i][J] = v;
#pragma unroll
			for (int c = J + 1; c < QR_PW; ++c)
				if (c < w)
					x[i][c] += kc[c] * v;
		}
	}
	if (g == 0 && tid == J) { // row J itself
		x[0][J] = -signed_norm;
#pragma unroll
		for (int c = J + 1; c < QR_PW; ++c)
			if (c < w)
				x[0][c] += kc[c];
	}
	__syncthreads();
	return true;
}

template <typename T, int RPT, int J> struct Qr2Steps {
	static __device__ __forceinline__ bool run(const QrPanelArgs<T> &a, T (&x)[RPT][QR_PW], Qr2Shared<T> &sh, int r0, int G, int &bar,
						   int &why, int steps)
	{
		if constexpr (J < QR_PW) {
			if (J >= steps)
				return true;
			if (!qr2_step<T, RPT, J>(a, x, sh, r0, G, bar, why))
				return false;
			return Qr2Steps<T, RPT, J + 1>::run(a, x, sh, r0, G, bar, why, steps);
		} else {
			return true;
		}
	}
};

template <typename T, int RPT> __global__ __launch_bounds__(QR2_NT) void qr_panel2_kernel(const QrPanelArgs<T> a)
{
	__shared__ Qr2Shared<T> sh;
	constexpr int R = QR2_NT * RPT;
	const int tid = threadIdx.x;
	const int g = blockIdx.x, G = gridDim.x;
	const int r0 = g * R;
	const int w = a.w;
	if (a.status[3] != 0)
		return; // an earlier panel found a rank deficiency: the whole factorization is being abandoned
	T x[RPT][QR_PW];
#pragma unroll
	for (int i = 0; i < RPT; ++i) {
		const int gr = r0 + tid + i * QR2_NT;
#pragma unroll
		for (int c = 0; c < QR_PW; ++c) {
			const bool in = gr < a.m && c < w;
			const T v = a.P[in ? (idx_t) gr * a.rs + (idx_t) c * a.cs : (idx_t) 0];
			x[i][c] = in ? v : (T) 0;
		}
	}
	const int steps = min(w, a.m);
	int bar = 0, why = 0;
	if (!Qr2Steps<T, RPT, 0>::run(a, x, sh, r0, G, bar, why, steps)) {
		if (tid == 0)
			atomicExch(a.status + why, 1);
		return;
	}
	// ---- T block: T_ij = v_i[j] + sum_{r > j} v_ri v_rj  (i < j) ; T_jj = tau_j
	{
		const int q = bar & 1;
		double acc2[QR_NPAIR];
#pragma unroll
		for (int p = 0; p < QR_NPAIR; ++p)
			acc2[p] = 0.0;
#pragma unroll
		for (int i = 0; i < RPT; ++i) {
			const int gr = r0 + tid + i * QR2_NT;
			if (gr < a.m) {
				int p = 0;
#pragma unroll
				for (int jj = 1; jj < QR_PW; ++jj)
#pragma unroll
					for (int ii = 0; ii < jj; ++ii, ++p)
						if (gr > jj && jj < w)
							acc2[p] += (double) x[i][ii] * (double) x[i][jj];
			}
		}
		block_sum<QR2_NT, QR_NPAIR>(acc2, sh.part, sh.red);
		// rows 0..7 of chunk 0 (V's top block) for the v_i[j] terms
		if (g == 0 && tid < QR_PW) {
#pragma unroll
			for (int c = 0; c < QR_PW; ++c)
				sh.top[tid][c] = x[0][c];
		}
		if (G > 1) {
			if (tid < QR_NPAIR)
				xwg_store(a.slots + ((size_t) q * G + g) * QR_SLOT + tid, sh.red[tid]);
			if (tid < 64)
				xwg_publish(a.flags, g, a.epoch_base + (xwg_u64) (bar + 1), tid == 0);
			if (!xwg_wait_all(a.flags, G, a.epoch_base + (xwg_u64) (bar + 1), &sh.flag)) {
				if (tid == 0)
					atomicExch(a.status + 2, 1);
				return;
			}
			double tot[QR_NPAIR];
#pragma unroll
			for (int p = 0; p < QR_NPAIR; ++p)
				tot[p] = 0.0;
			if (g == 0) {
				for (int t = tid; t < G; t += QR2_NT)
#pragma unroll
					for (int p = 0; p < QR_NPAIR; ++p)
						tot[p] += xwg_load(a.slots + ((size_t) q * G + t) * QR_SLOT + p);
				block_sum<QR2_NT, QR_NPAIR>(tot, sh.part, sh.red);
			}
		}
		__syncthreads();
		if (g == 0 && tid == 0) {
			int p = 0;
			for (int jj = 0; jj < w; ++jj)
				a.Tb[(idx_t) jj * a.trs + (idx_t) jj * a.tcs] = (T) sh.tau[jj];
			for (int jj = 1; jj < QR_PW; ++jj)
				for (int ii = 0; ii < jj; ++ii, ++p)
					if (jj < w)
						a.Tb[(idx_t) ii * a.trs + (idx_t) jj * a.tcs] = (T) ((double) sh.top[jj][ii] + sh.red[p]);
		}
	}
#pragma unroll
	for (int i = 0; i < RPT; ++i) {
		const int gr = r0 + tid + i * QR2_NT;
#pragma unroll
		for (int c = 0; c < QR_PW; ++c)
			if (gr < a.m && c < w)
				a.P[(idx_t) gr * a.rs + (idx_t) c * a.cs] = x[i][c];
	}
}

template <typename T> struct QrWork {
	double *slots, *head;
	xwg_u64 *flags, *gran, *gran_head;
	xwg_u64 epoch_base;
	int *status;
	const T *a_top; // A[0, 0]
	idx_t rs, cs;
};

template <typename T> static constexpr int qr_rmax() { return sizeof(T) == 8 ? 2240 : 4480; }

template <typename T> static void qr_leaf(MatV<T> P, MatV<T> Tb, idx_t row_abs, idx_t col_abs, QrWork<T> &wk)
{
	constexpr int R = QR2_NT * qr2_rpt<T>();
	const idx_t m = P.nrows;
	const int w = (int) P.ncols;
	int G = (int) ((m + R - 1) / R);
	if (G < 1)
		G = 1;
	FH_CHECK(G <= QR_GMAX, "qr: panel too tall for the cooperative kernel");
	QrPanelArgs<T> a;
	a.P = P.p;
	a.rs = P.rs;
	a.cs = P.cs;
	a.m = (int) m;
	a.w = w;
	a.R = R;
	a.above = wk.a_top + col_abs * wk.cs;
	a.row_abs = (int) row_abs;
	a.Tb = Tb.p;
	a.trs = Tb.rs;
	a.tcs = Tb.cs;
	a.slots = wk.slots;
	a.head = wk.head;
	a.flags = wk.flags;
	a.gran = wk.gran;
	a.gran_head = wk.gran_head;
	a.epoch_base = wk.epoch_base;
	a.status = wk.status;
	hipLaunchKernelGGL((qr_panel2_kernel<T, qr2_rpt<T>()>), dim3(G), dim3(QR2_NT), 0, ctx().stream, a);
	FH_HIP(hipGetLastError());
	if (G > 1) {
		const int steps = w < (int) m ? w : (int) m;
		wk.epoch_base += (xwg_u64) (steps + 1);
	}
}

// P: rows from the diagonal row of its first column; Tb: w x w block of Q_coeff
template <typename T> static void qr_rec(MatV<T> P, MatV<T> Tb, idx_t row_abs, idx_t col_abs, QrWork<T> &wk)
{
	const idx_t m = P.nrows, w = P.ncols;
	if (w == 0 || m == 0)
		return;
	if (w <= QR_PW) {
		qr_leaf<T>(P, Tb, row_abs, col_abs, wk);
		return;
	}
	// A panel of up to 64 columns that is tall enough takes the one-pass panel (tsqr.hip): Gram matrix, ONE small kernel, V = P M --
	// instead of 8 cooperative leaves (one all-reduce per column) and the level-3 steps between them.  A panel it refuses (ill
	// conditioned, a column failing the reference's rank test, ...) is untouched and goes down the recursion as before.
	const bool onepass_tall = P.nrows >= 256;
	bool first_done = false; // a 128-column node whose first panel the one-pass path completed (and applied to the second) before it stopped
	if ((w <= 64 || w == 128) && tsqr_panel_applicable<T>(m, w, P.rs, P.cs)) {
		Scratch taus((size_t) w * sizeof(T));
		int reason = 0;
		// (rows above the panel in the parent count in the rank test: row_abs of them)
		const idx_t done = tsqr_factor<T>(P, MatV<T>{Tb.p, w, w, Tb.rs, Tb.cs}, taus.as<T>(), &reason, row_abs);
		if (done == w)
			return;
		first_done = w == 128 && done == 64; // T11 is complete (one panel), the second panel is untouched but updated
	}
	idx_t w1 = ((w / 2 + QR_PW - 1) / QR_PW) * QR_PW;
	if (w1 >= w)
		w1 = w - QR_PW;
	if (onepass_tall && w > 64) {
		// split at a multiple of 64 so that both halves end in whole one-pass panels where they can
		w1 = ((w / 2 + 63) / 64) * 64;
		if (w1 >= w)
			w1 = w - 64;
	}
	if (first_done)
		w1 = 64;
	const idx_t w2 = w - w1;
	MatV<T> V1 = P.sub(0, 0, m, w1), B = P.sub(0, w1, m, w2);
	MatV<T> T11 = Tb.sub(0, 0, w1, w1), T12 = Tb.sub(0, w1, w1, w2), T22 = Tb.sub(w1, w1, w2, w2);
	if (!first_done) {
		qr_rec<T>(V1, T11, row_abs, col_abs, wk);
		apply_block_householder_dev<T>(V1.c(), T11.c(), B, true); // factor.rs:241-249
	}
	if (m > w1) {
		MatV<T> P2 = P.sub(w1, w1, m - w1, w2);
		qr_rec<T>(P2, T22, row_abs + w1, col_abs + w1, wk);
		// T12 = V1[w1:, :]^H V2 (householder.rs:249-267): V2 unit lower trapezoidal (m - w1) x w2
		const idx_t mt = m - w1;
		const idx_t top = mt < w2 ? mt : w2;
		MatV<const T> V1m = P.sub(w1, 0, top, w1).c(), V2top = P.sub(w1, w1, top, w2).c();
		// rectangular (w1 x top) times unit-lower-trapezoidal top block: treat the top x w2 block as
		// [unit lower | 0]; when mt < w2 only the leading mt x mt part is triangular
		if (top == w2) {
			matmul_triangular_dev<T>(T12, 0, false, V1m.t(), 0, V2top, 5, (T) 1);
			if (mt > w2)
				gemm_dev<T>(T12, DST_FULL, true, P.sub(w1 + w2, 0, mt - w2, w1).c().t(),
					    P.sub(w1 + w2, w1, mt - w2, w2).c(), (T) 1);
		} else {
			FH_CHECK(false, "qr: internal: wide panel in the fast path");
		}
	}
}

// ------------------------------------------------------------------------------------------------
// GENERAL path: qr_in_place_unblocked (factor.rs:11-86) with `row` kept on the device
// ------------------------------------------------------------------------------------------------
struct GqState {
	int row;     // accepted reflectors so far
	int lim;     // min(size, m)
	int mode;    // 1: the scaled tail is written this column
	int apply;   // 1: update the remaining columns
	int accept;  // 1: row += 1 afterwards
	int active;  // 0 once row reached lim
	double acc[6]; // scaled sums: above {sml, med, big}, tail {sml, med, big}
	double hinv, tau_inv;
};

template <typename T> struct GqArgs {
	T *A;
	idx_t rs, cs;
	int m, n, col;
	GqState *st;
	double *dots; // n entries
	double *kvec; // n entries
	T *taus;      // size entries
	int top;      // rows of a parent matrix ABOVE A(0, :) that belong to the columns as well (they count in the rank test)
};

// reductions/norm_l2.rs:6-45: three accumulators of (x*sml)^2, x^2, (x*big)^2, in the scalar type
template <typename T> __global__ void gq_norms_kernel(const GqArgs<T> a)
{
	__shared__ double s_part[4 * 6], s_red[6];
	const int row = a.st->row;
	if (row >= a.st->lim)
		return;
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T acc[6] = {0, 0, 0, 0, 0, 0};
	// (i < 0: the column's entries in the parent's rows above this submatrix -- factor.rs:26,52-58 takes the norm of ALL rows above)
	for (int i = -a.top + (int) (blockIdx.x * blockDim.x + threadIdx.x); i < a.m; i += gridDim.x * blockDim.x) {
		if (i == row)
			continue;
		const T x = a.A[(idx_t) i * a.rs + (idx_t) a.col * a.cs];
		const int o = i < row ? 0 : 3;
		acc[o + 0] += (x * sml) * (x * sml);
		acc[o + 1] += x * x;
		acc[o + 2] += (x * big) * (x * big);
	}
	double accd[6];
	for (int k = 0; k < 6; ++k)
		accd[k] = (double) acc[k];
	block_sum<256, 6>(accd, s_part, s_red);
	if (threadIdx.x < 6)
		atomicAdd(&a.st->acc[threadIdx.x], s_red[threadIdx.x]);
}

template <typename T> __global__ void gq_house_kernel(const GqArgs<T> a)
{
	GqState *st = a.st;
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	const int row = st->row;
	st->mode = 0;
	st->apply = 0;
	st->accept = 0;
	st->active = row < st->lim ? 1 : 0;
	if (!st->active)
		return;
	const T norm_above = norm_from3<T>(st->acc);
	const T tail_norm = norm_from3<T>(st->acc + 3);
	for (int k = 0; k < 6; ++k)
		st->acc[k] = 0.0;
	T *hp = a.A + (idx_t) row * a.rs + (idx_t) a.col * a.cs;
	T head = *hp;
	T head_norm = fabs(head);
	T tau, inorm;
	if (head_norm < Lim<T>::minpos) { // householder.rs:66-69
		head = (T) 0;
		head_norm = (T) 0;
		*hp = head;
	}
	if (tail_norm < Lim<T>::minpos) { // householder.rs:70-77
		tau = std::numeric_limits<T>::infinity();
		inorm = head_norm;
	} else {
		const T norm = (T) hypot((double) head_norm, (double) tail_norm);
		const T sign = head_norm != (T) 0 ? head * ((T) 1 / head_norm) : (T) 1;
		const T signed_norm = sign * norm;
		const T hinv = (T) 1 / (head + signed_norm);
		*hp = -signed_norm;
		const T tn = tail_norm * fabs(hinv);
		tau = (T) 0.5 * ((T) 1 + tn * tn);
		inorm = norm;
		st->hinv = (double) hinv;
		st->mode = 1;
	}
	const T full = (T) hypot((double) inorm, (double) norm_above);
	const T threshold = Lim<T>::eps * (T) ((double) (a.m - row) * 16.0) * full;
	const T tau_inv = (T) 1 / tau;
	a.taus[row] = tau; // H[row] = tau (factor.rs:57)
	st->tau_inv = (double) tau_inv;
	if (tau_inv < Lim<T>::minpos) {
		if (inorm > (T) 0)
			st->accept = 1;
	} else if (inorm > threshold) {
		st->apply = 1;
		st->accept = 1;
	}
}

// v = tail * hinv written into column `row` (in place when row == col); when row != col the first
// min(len, col - row) entries of the original tail are zeroed (factor.rs:39-50)
template <typename T> __global__ void gq_scale_kernel(const GqArgs<T> a)
{
	const GqState *st = a.st;
	if (!st->active)
		return;
	const int row = st->row, col = a.col;
	const T hinv = (T) st->hinv;
	for (int i = row + 1 + blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += gridDim.x * blockDim.x) {
		T *src = a.A + (idx_t) i * a.rs + (idx_t) col * a.cs;
		if (st->mode == 1)
			a.A[(idx_t) i * a.rs + (idx_t) row * a.cs] = *src * hinv;
		if (row != col && i - (row + 1) < col - row)
			*src = (T) 0;
	}
}

template <typename T> __global__ void gq_dots_kernel(const GqArgs<T> a)
{
	__shared__ double s_part[4], s_red[1];
	const GqState *st = a.st;
	if (!st->active || !st->apply)
		return;
	const int row = st->row;
	const int c = a.col + 1 + blockIdx.y;
	double acc[1] = {0.0};
	for (int i = row + 1 + blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += gridDim.x * blockDim.x)
		acc[0] += (double) a.A[(idx_t) i * a.rs + (idx_t) row * a.cs] * (double) a.A[(idx_t) i * a.rs + (idx_t) c * a.cs];
	block_sum<256, 1>(acc, s_part, s_red);
	if (threadIdx.x == 0)
		atomicAdd(&a.dots[c], s_red[0]);
}

template <typename T> __global__ void gq_heads_kernel(const GqArgs<T> a)
{
	const GqState *st = a.st;
	const int c = a.col + 1 + blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= a.n)
		return;
	if (st->active && st->apply) {
		T *hp = a.A + (idx_t) st->row * a.rs + (idx_t) c * a.cs;
		const T dot = *hp + (T) a.dots[c];
		const T k = -(dot * (T) st->tau_inv);
		*hp += k;
		a.kvec[c] = (double) k;
	}
	a.dots[c] = 0.0;
}

template <typename T> __global__ void gq_update_kernel(const GqArgs<T> a)
{
	const GqState *st = a.st;
	if (!st->active || !st->apply)
		return;
	const int row = st->row;
	const int c = a.col + 1 + blockIdx.y;
	const T k = (T) a.kvec[c];
	for (int i = row + 1 + blockIdx.x * blockDim.x + threadIdx.x; i < a.m; i += gridDim.x * blockDim.x)
		a.A[(idx_t) i * a.rs + (idx_t) c * a.cs] += k * a.A[(idx_t) i * a.rs + (idx_t) row * a.cs];
}

__global__ void gq_advance_kernel(GqState *st)
{
	if (st->active && st->accept)
		st->row += 1;
}

template <typename T> static long qr_general(MatV<T> A, T *taus_dev, idx_t top = 0)
{
	const idx_t m = A.nrows, n = A.ncols;
	const idx_t size = m < n ? m : n;
	hipStream_t s = ctx().stream;
	Scratch stb(sizeof(GqState)), dotsb((size_t) n * 8 + 8), kb((size_t) n * 8 + 8);
	FH_HIP(hipMemsetAsync(stb.p, 0, sizeof(GqState), s));
	FH_HIP(hipMemsetAsync(dotsb.p, 0, (size_t) n * 8 + 8, s));
	GqState init;
	memset(&init, 0, sizeof(init));
	init.lim = (int) size;
	FH_HIP(hipMemcpyAsync(stb.p, &init, sizeof(init), hipMemcpyHostToDevice, s));
	FH_HIP(hipStreamSynchronize(s)); // `init` lives on the stack
	GqArgs<T> a;
	a.A = A.p;
	a.rs = A.rs;
	a.cs = A.cs;
	a.m = (int) m;
	a.n = (int) n;
	a.st = stb.as<GqState>();
	a.dots = dotsb.as<double>();
	a.kvec = kb.as<double>();
	a.taus = taus_dev;
	a.top = (int) top;
	int rb = (int) ((m + 255) / 256);
	if (rb > 1024)
		rb = 1024;
	if (rb < 1)
		rb = 1;
	for (idx_t col = 0; col < n; ++col) {
		a.col = (int) col;
		const int rem = (int) (n - col - 1);
		hipLaunchKernelGGL(gq_norms_kernel<T>, dim3(rb), dim3(256), 0, s, a);
		hipLaunchKernelGGL(gq_house_kernel<T>, dim3(1), dim3(64), 0, s, a);
		hipLaunchKernelGGL(gq_scale_kernel<T>, dim3(rb), dim3(256), 0, s, a);
		if (rem > 0) {
			for (int c0 = 0; c0 < rem; c0 += 32768) {
				GqArgs<T> b = a;
				b.col = (int) col + c0; // columns col+1+c0 ...
				const int nc = rem - c0 < 32768 ? rem - c0 : 32768;
				// dots/update index columns relative to b.col; `row`/v come from the state
				hipLaunchKernelGGL(gq_dots_kernel<T>, dim3(rb, nc), dim3(256), 0, s, b);
			}
			hipLaunchKernelGGL(gq_heads_kernel<T>, dim3((rem + 255) / 256), dim3(256), 0, s, a);
			for (int c0 = 0; c0 < rem; c0 += 32768) {
				GqArgs<T> b = a;
				b.col = (int) col + c0;
				const int nc = rem - c0 < 32768 ? rem - c0 : 32768;
				hipLaunchKernelGGL(gq_update_kernel<T>, dim3(rb, nc), dim3(256), 0, s, b);
			}
		}
		hipLaunchKernelGGL(gq_advance_kernel, dim3(1), dim3(1), 0, s, a.st);
	}
	FH_HIP(hipGetLastError());
	GqState fin;
	FH_HIP(hipMemcpyAsync(&fin, stb.p, sizeof(fin), hipMemcpyDeviceToHost, s));
	FH_HIP(hipStreamSynchronize(s));
	return fin.row;
}

// Q_coeff post-processing.  mode 0: write T_jj = taus[j] for j < rank (general path);
// always: Q_coeff[:, rank..] = 0 and the +inf diagonal of factor.rs:287-299.
template <typename T>
__global__ void qr_finalize_kernel(T *H, idx_t hrs, idx_t hcs, int bs, int size, int rank, const T *taus, int write_tau)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= size)
		return;
	if (j < rank) {
		if (write_tau)
			H[(idx_t) (j % bs) * hrs + (idx_t) j * hcs] = taus[j];
		return;
	}
	for (int i = 0; i < bs; ++i)
		H[(idx_t) i * hrs + (idx_t) j * hcs] = (T) 0;
	// block containing j starts at col0 = j / bs * bs; the diagonal entries from max(rank, col0) on are +inf
	const int col0 = j / bs * bs;
	if (col0 >= rank / bs * bs) {
		const int start = rank > col0 ? rank : col0;
		if (j >= start)
			H[(idx_t) (j - col0) * hrs + (idx_t) j * hcs] = std::numeric_limits<T>::infinity();
	}
}

// T blocks over the first `rank` reflectors from their taus: striu(V^H V) (householder.rs:185-209), diagonal = tau;
// the columns from `rank` on get the zero / +inf pattern of factor.rs:287-299
// striu(V_b^H V_b) of EVERY block of reflectors in one launch (one workgroup per block): the blocks are independent, and
// one block is a 32 x 32 .. 64 x 64 Gram matrix over up to m rows -- as separate split-K GEMM launches they were 127 x
// 118 us = 15 ms of every N = 4096 reduction to condensed form.  Rows in chunks through LDS with the unit-lower structure
// applied on the way in (zeros above the diagonal, 1 on it), sums in fp64 in ascending row order.
// (round 6: a second instantiation for blocks of up to 128 reflectors -- the recommended block size from 2048^2 entries on -- with 512 threads:
// the column-pivot QR at N = 4096 spent 9 of its 134 ms in 126 per-block GEMM launches)
constexpr int TB_ROWS = 32;
template <typename T, int TB_MAXW, int TB_NT>
__global__ __launch_bounds__(TB_NT) void qr_tblock_gram_kernel(const T *V, idx_t vrs, idx_t vcs, int m, int rank, int bs, T *H, idx_t hrs, idx_t hcs)
{
	__shared__ T L[TB_ROWS][TB_MAXW + 1];
	const int tid = threadIdx.x;
	const int c0 = blockIdx.x * bs;
	const int wb = min(bs, rank - c0);
	const int npairs = wb * (wb - 1) / 2;
	constexpr int MAXP = (TB_MAXW * (TB_MAXW - 1) / 2 + TB_NT - 1) / TB_NT;
	double acc[MAXP];
	int pi[MAXP], pj[MAXP];
#pragma unroll
	for (int q = 0; q < MAXP; ++q) {
		acc[q] = 0.0;
		const int p = tid + q * TB_NT;
		// pair p -> (i < j), enumerated column by column: j = 1: (0,1); j = 2: (0,2), (1,2); ...
		int j = 1;
		if (p < npairs) {
			j = (int) ((1.0f + sqrtf(1.0f + 8.0f * (float) p)) * 0.5f);
			while (j * (j - 1) / 2 > p)
				--j;
			while ((j + 1) * j / 2 <= p)
				++j;
		}
		pj[q] = j;
		pi[q] = p < npairs ? p - j * (j - 1) / 2 : 0;
	}
	const int rows = m - c0; // rows of this block's reflectors
	for (int r0 = 0; r0 < rows; r0 += TB_ROWS) {
		__syncthreads();
		for (int e = tid; e < TB_ROWS * wb; e += TB_NT) {
			const int c = e / TB_ROWS, rr = e - c * TB_ROWS, r = r0 + rr; // lanes along the rows (unit stride for column-major V)
			T v = (T) 0;
			if (r < rows)
				v = r < c ? (T) 0 : (r == c ? (T) 1 : V[(idx_t) (c0 + r) * vrs + (idx_t) (c0 + c) * vcs]);
			L[rr][c] = v;
		}
		__syncthreads();
#pragma unroll
		for (int q = 0; q < MAXP; ++q) {
			if (tid + q * TB_NT < npairs) {
				double t = acc[q];
#pragma unroll 8
				for (int rr = 0; rr < TB_ROWS; ++rr)
					t += (double) L[rr][pi[q]] * (double) L[rr][pj[q]];
				acc[q] = t;
			}
		}
	}
#pragma unroll
	for (int q = 0; q < MAXP; ++q)
		if (tid + q * TB_NT < npairs)
			H[(idx_t) pi[q] * hrs + (idx_t) (c0 + pj[q]) * hcs] = (T) acc[q];
}

template <typename T> void qr_t_blocks_from_taus(MatV<T> A, MatV<T> H, idx_t rank, const T *taus)
{
	const idx_t m = A.nrows, n = A.ncols, bs = H.nrows;
	const idx_t size = m < n ? m : n;
	const bool batched = true; // (one split-K GEMM per block was 15 ms of every N = 4096 reduction: DESIGN.md 3.8)
	if (batched && bs <= 128 && rank > 0) {
		if (bs > 64)
			hipLaunchKernelGGL((qr_tblock_gram_kernel<T, 128, 512>), dim3((unsigned) ((rank + bs - 1) / bs)), dim3(512), 0, ctx().stream, A.p, A.rs, A.cs,
					   (int) m, (int) rank, (int) bs, H.p, H.rs, H.cs);
		else if (bs > 1)
			hipLaunchKernelGGL((qr_tblock_gram_kernel<T, 64, 256>), dim3((unsigned) ((rank + bs - 1) / bs)), dim3(256), 0, ctx().stream, A.p, A.rs, A.cs,
					   (int) m, (int) rank, (int) bs, H.p, H.rs, H.cs);
		FH_HIP(hipGetLastError());
	} else {
		for (idx_t c0 = 0; c0 < rank; c0 += bs) {
			const idx_t wb = bs < rank - c0 ? bs : rank - c0;
			MatV<T> Tb = H.sub(0, c0, wb, wb);
			MatV<const T> Vtop = A.sub(c0, c0, wb, wb).c();
			matmul_triangular_dev<T>(Tb, 6, false, Vtop.t(), 6, Vtop, 5, (T) 1);
			if (m - c0 > wb) {
				MatV<const T> Vbot = A.sub(c0 + wb, c0, m - c0 - wb, wb).c();
				GemmExtra<T> ex;
				ex.dst_strict = true;
				gemm_dev<T>(Tb, DST_UPPER, true, Vbot.t(), Vbot, (T) 1, &ex);
			}
		}
	}
	hipLaunchKernelGGL(qr_finalize_kernel<T>, dim3((unsigned) ((size + 255) / 256)), dim3(256), 0, ctx().stream, H.p, H.rs, H.cs, (int) bs,
			   (int) size, (int) rank, taus, 1);
	FH_HIP(hipGetLastError());
}
template void qr_t_blocks_from_taus<double>(MatV<double>, MatV<double>, idx_t, const double *);
template void qr_t_blocks_from_taus<float>(MatV<float>, MatV<float>, idx_t, const float *);

// ------------------------------------------------------------------------------------------------
// drivers
// ------------------------------------------------------------------------------------------------
// Backup copy of A for the fast path, fused with the range guard of the fp64 fast path: the cooperative leaf
// accumulates PLAIN squares and dot products in fp64 (exact for fp32 data, whose squares cannot leave the fp64
// range), whereas the reference's norm_l2 keeps three differently scaled accumulators
// (reductions/norm_l2.rs:6-45,173-184) and stays accurate for |x| ~ 1e+-250.  fp64 data with a non-zero entry
// outside [1e-120, 1e120] (or a non-finite one) therefore raises the "abandon the fast path" flag and the
// factorization runs on the general path, which restates norm_l2 literally.
template <typename T>
__global__ void copy_guard_kernel(T *d, idx_t drs, idx_t dcs, const T *s, idx_t srs, idx_t scs, idx_t M, idx_t N, int *flag)
{
	const idx_t total = M * N;
	bool bad = false;
	for (idx_t e = (idx_t) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (idx_t) gridDim.x * blockDim.x) {
		const idx_t i = e % M, j = e / M;
		const T v = s[i * srs + j * scs];
		d[i * drs + j * dcs] = v;
		if constexpr (sizeof(T) == 8) {
			const double av = fabs((double) v);
			bad = bad || (av != 0.0 && !(av >= 1e-120 && av <= 1e120));
		}
	}
	if (__any(bad) && (threadIdx.x & 63) == 0)
		atomicExch(flag, 1);
}

// `off` > 0: A is the trailing part parent(off:, off:) of a matrix whose first `off` columns are finished reflectors (the
// one-pass path stopped there).  The reference's rank test looks at a column's entries in ALL rows above the current one
// (factor.rs:26,52-58), so the `off` parent rows above A count: both paths below read them through negative row offsets.
template <typename T> static long geqrf_classic(MatV<T> A, MatV<T> H, idx_t blocking_threshold, idx_t off = 0)
{
	(void) blocking_threshold; // the GPU recursion always blocks; leaves are 8 columns wide
	const idx_t m = A.nrows, n = A.ncols;
	const idx_t size = m < n ? m : n;
	const idx_t bs = H.nrows;
	FH_CHECK(bs > 0 && H.ncols == size, "qr: Q_coeff must be block_size x min(nrows, ncols)");
	FH_CHECK(m < (1L << 30) && n < (1L << 30), "qr: matrix too large");
	if (size == 0)
		return 0;
	hipStream_t s = ctx().stream;
	Scratch misc(256);
	FH_HIP(hipMemsetAsync(misc.p, 0, 256, s));
	int *status = misc.as<int>() + 8;
	long rank = -1;

	// The reference's rank test (factor.rs:52-58) accepts column 0 only if norm > eps * 16 * m * norm, i.e. it
	// rejects EVERY column once 16 * eps * nrows >= 1 (fp32: nrows >= 524288).  That outcome (rank 0) is
	// reproduced by the general path; the fast path would only discover it one launch later.
	const bool ref_rejects_all = (double) Lim<T>::eps * 16.0 * (double) m >= 1.0;
	// the cooperative leaf needs all its workgroups resident: one 512-thread workgroup per CU at its register footprint
	hipDeviceProp_t prop;
	FH_HIP(hipGetDeviceProperties(&prop, ctx().device));
	const idx_t gcap = prop.multiProcessorCount < QR_GMAX ? prop.multiProcessorCount : QR_GMAX;
	const bool fast_ok = m <= (idx_t) QR2_NT * qr2_rpt<T>() * gcap && !ref_rejects_all;
	Scratch backup(fast_ok ? (size_t) m * (size_t) n * sizeof(T) : 256);
	MatV<T> Bk{backup.as<T>(), m, n, 1, m};
	if (fast_ok) {
		{
			const idx_t total = m * n;
			idx_t blocks = (total + 255) / 256;
			if (blocks > 65536)
				blocks = 65536;
			MatV<T> Ad = A, Bd = Bk;
			auto ab = [](idx_t x) { return x < 0 ? -x : x; };
			if (ab(Ad.cs) < ab(Ad.rs)) { // fast index along the smaller stride
				Ad = Ad.t();
				Bd = Bd.t();
			}
			hipLaunchKernelGGL(copy_guard_kernel<T>, dim3((unsigned) blocks), dim3(256), 0, s, Bd.p, Bd.rs, Bd.cs, Ad.p, Ad.rs, Ad.cs,
					   Ad.nrows, Ad.ncols, status + 3);
			FH_HIP(hipGetLastError());
		}
		Scratch slots((size_t) 2 * QR_GMAX * QR_SLOT * sizeof(double)), head((size_t) 2 * (QR_PW + 1) * sizeof(double));
		QrWork<T> wk;
		wk.slots = slots.as<double>();
		wk.head = head.as<double>();
		Scratch flagb((size_t) QR_GMAX * sizeof(xwg_u64));
		FH_HIP(hipMemsetAsync(flagb.p, 0, (size_t) QR_GMAX * sizeof(xwg_u64), s));
		wk.flags = flagb.as<xwg_u64>();
		const size_t gran_n = (size_t) 2 * QR_GMAX * 2 * QR_PW + (size_t) 2 * 2 * (QR_PW + 1);
		Scratch granb(gran_n * sizeof(xwg_u64));
		FH_HIP(hipMemsetAsync(granb.p, 0, gran_n * sizeof(xwg_u64), s));
		wk.gran = granb.as<xwg_u64>();
		wk.gran_head = wk.gran + (size_t) 2 * QR_GMAX * 2 * QR_PW;
		wk.epoch_base = 0;
		wk.status = status;
		wk.a_top = A.p - off * A.rs - off * A.cs; // origin of the parent
		wk.rs = A.rs;
		wk.cs = A.cs;
		for (idx_t c0 = 0; c0 < size; c0 += bs) {
			const idx_t wb = bs < size - c0 ? bs : size - c0;
			MatV<T> P = A.sub(c0, c0, m - c0, wb);
			MatV<T> Tb = H.sub(0, c0, wb, wb);
			qr_rec<T>(P, Tb, off + c0, off + c0, wk);
			if (c0 + wb < n) // factor.rs:241-249: apply Q_k^H to everything on the right
				apply_block_householder_dev<T>(P.c(), Tb.c(), A.sub(c0, c0 + wb, m - c0, n - c0 - wb), true);
		}
		int st[4];
		FH_HIP(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
		if (st[2] != 0) // the cooperative leaf did not get all its workgroups resident in time (GPU shared with other work):
			fprintf(stderr, "faer_hip: qr: the cross-workgroup exchange of the panel kernel timed out; redoing on the general path\n");
		if (st[2] == 0 && st[3] == 0)
			rank = (long) size;
		else
			copy_dev<T>(A, Bk.c()); // rank deficient (or timed out): redo from the saved copy on the general path
	}
	if (rank < 0) {
		Scratch taus((size_t) size * sizeof(T));
		rank = qr_general<T>(A, taus.as<T>(), off);
		qr_t_blocks_from_taus<T>(A, H, rank, taus.as<T>());
		FH_HIP(hipStreamSynchronize(s)); // taus scratch is released on return
	}
	return rank;
}

template <typename T> __global__ void qr_taus_from_blocks_kernel(const T *H, idx_t hrs, idx_t hcs, int bs, int count, T *taus)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < count)
		taus[j] = H[(idx_t) (j % bs) * hrs + (idx_t) j * hcs];
}

// Tall matrices take the one-pass path (tsqr.hip; fp64 since the end of round 6).  It stops in front of the first 64-column panel it cannot
// take (ill conditioned, a column failing the reference's rank test, ...) with every earlier reflector applied to
// everything on its right -- the state qr_in_place_blocked (factor.rs:137-256) is in at that column -- so the classic
// path simply factors the remaining submatrix and the T blocks are rebuilt from V and the taus.
static thread_local long g_qr_one_pass_columns = -1; // of this thread's last QR: columns the one-pass path completed, -1 = not taken
long qr_last_one_pass_columns() { return g_qr_one_pass_columns; }

template <typename T> long geqrf_dev(MatV<T> A, MatV<T> H, idx_t blocking_threshold)
{
	g_qr_one_pass_columns = -1;
	{
		const idx_t m = A.nrows, n = A.ncols, bs = H.nrows;
		const idx_t size = m < n ? m : n;
		const bool ref_rejects_all = (double) Lim<T>::eps * 16.0 * (double) m >= 1.0;
		// A block size of Q_coeff that neither divides a 64-column panel nor is a multiple of it (faer recommends 48 for many moderately
		// tall shapes): the path runs with 64-column blocks of its own and the caller's blocks are rebuilt from V and the taus (one
		// batched Gram launch over V: one workgroup per block walks all rows -- 8192 x 64 with blocks of 48: 1.2 ms of rebuild against
		// 0.44 ms for the whole classic factorization -- so only up to 3072 rows: tools/gpu_qr_shape_rule.py).
		const bool bs_direct = bs > 0 && (bs % 64 == 0 || 64 % bs == 0);
		if (size > 0 && bs > 0 && H.ncols == size && !ref_rejects_all && (bs_direct || m <= 3072) && tsqr_applicable<T>(A, bs_direct ? bs : 64)) {
			Scratch taus((size_t) size * sizeof(T));
			Scratch hown(bs_direct ? 256 : (size_t) 64 * (size_t) size * sizeof(T));
			int reason = 0;
			const idx_t done = tsqr_factor<T>(A, bs_direct ? H : MatV<T>{hown.as<T>(), 64, size, 1, 64}, taus.as<T>(), &reason);
			g_qr_one_pass_columns = (long) done;
			if (done == size) {
				if (!bs_direct) {
					qr_t_blocks_from_taus<T>(A, H, size, taus.as<T>());
					FH_HIP(hipStreamSynchronize(ctx().stream)); // scratch is released on return
				}
				return (long) size;
			}
			static const bool verbose = getenv("FAER_HIP_VERBOSE") != nullptr;
			if (verbose)
				fprintf(stderr, "faer_hip: qr: one-pass path stopped at column %ld (reason %d); classic path for the rest\n", (long) done, reason);
			MatV<T> B = A.sub(done, done, m - done, n - done);
			const idx_t size2 = size - done;
			Scratch h2((size_t) bs * (size_t) size2 * sizeof(T));
			MatV<T> H2{h2.as<T>(), bs, size2, 1, bs};
			fill_dev<T>(H2, DST_FULL, (T) 0);
			const long r2 = geqrf_classic<T>(B, H2, blocking_threshold, done);
			if (r2 > 0) {
				hipLaunchKernelGGL(qr_taus_from_blocks_kernel<T>, dim3((unsigned) ((r2 + 255) / 256)), dim3(256), 0, ctx().stream, H2.p, H2.rs, H2.cs,
						   (int) bs, (int) r2, taus.as<T>() + done);
				FH_HIP(hipGetLastError());
			}
			const long rank = (long) done + r2;
			qr_t_blocks_from_taus<T>(A, H, rank, taus.as<T>());
			FH_HIP(hipStreamSynchronize(ctx().stream)); // scratch is released on return
			return rank;
		}
	}
	return geqrf_classic<T>(A, H, blocking_threshold);
}

template long geqrf_dev<double>(MatV<double>, MatV<double>, idx_t);
template long geqrf_dev<float>(MatV<float>, MatV<float>, idx_t);
template void apply_householder_sequence_left_dev<double>(MatV<const double>, MatV<const double>, MatV<double>, bool);
template void apply_householder_sequence_left_dev<float>(MatV<const float>, MatV<const float>, MatV<float>, bool);

} // namespace fh
