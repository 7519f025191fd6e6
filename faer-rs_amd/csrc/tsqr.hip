// One-pass tall-skinny Householder QR for gfx950 (fp32 data; fp64 data: the section "fp64 data" further down): faer's (V, T, R) -- qr/no_pivoting/factor.rs:137-256,
// householder.rs:21-23,59-107,132-272 -- without a cross-workgroup reduction per column.
// Callers (qr.hip): geqrf_dev for whole matrices of >= 1024 rows and >= 3 rows per column (tsqr_applicable), and the
// classic path's recursion for single panels and two-panel nodes of any matrix (tsqr_panel_applicable, `rows_above`).
//
// The classic path (qr.hip) follows the reference's recursion: every column of a panel costs one device-wide
// all-reduce and every level of the recursion a handful of dependent launches; a 5e5 x 256 matrix is streamed
// dozens of times and nothing is bound by HBM or by the matrix cores.  Here the matrix is processed in 64-column
// panels with a constant number of launches per panel, every trailing column read and written once per panel:
//
//   gram    G = P^T P (fp64 matrix cores: products of fp32 data are exact in fp64) and C = P^T X (fp32 matrix cores,
//           per-workgroup partial sums added in fp64 in a fixed order) over the rows from the panel's diagonal down;
//           P = the 64 panel columns, X = the columns right of it.  Row chunks go through LDS; the row order inside
//           a chunk is irrelevant for a Gram sum, so operands are read back as 16-byte quads of consecutive rows.
//   panel   (one workgroup, fp64) R~ = chol(G)^T; Householder reconstruction on the top block A1 (Ballard, Demmel,
//           Grigori, Jacquelin, Nguyen, Solomonik: "Reconstructing Householder vectors from TSQR"): Q1~ = A1 R~^-1,
//           sign-choosing LU  I - Q1~ S = V1 U  (s_j = -sign of the pivot candidate: exactly the reference's
//           beta = -sign(x0) |x|, householder.rs:82-101), R = S R~, M = -(U R)^-1, T = V1^T U^-1
//           (= striu(V^T V) + diag(tau), the reference's factor with H = I - V T^-1 V^T).
//           Below the top block the reflectors are V = P M: one more product, no reduction.
//   y       D = R^-T C are the new top rows of X (= Q^T X), Y = R^-1 (V1 U)^-1 (D - X_top); below the top block the
//           block reflector applied to X is X - P Y (the raw panel again, not V).
//   update  X <- X - P Y and V = P M, fused with the next panel's Gram products (tq_fused_kernel); V = P M as a launch of its own
//           (tq_form_v_kernel) where nothing else carries it: rows are independent, so a wavefront maps ANY 32 rows to the 32
//           columns of a v_mfma_f32_32x32x2 tile -- each lane loads and stores 16-byte quads of its own rows straight
//           from / to HBM, no LDS on the streamed side.
//
// Accuracy: R comes from an fp64 Cholesky factor of an exactly accumulated Gram matrix: relative error
// ~ cond(panel)^2 * 2^-53, i.e. below fp32 rounding for cond(panel) < ~1e4 (measured on the CPU prototype
// tests/diag/proto_tsqr.py: closer to an fp64 Householder QR than the fp32 Householder QR is).  V = P M and D = R^-T C
// amplify fp32 rounding by cond(panel), so the panel kernel REFUSES a panel whose Frobenius condition estimate exceeds
// TQ_COND_MAX, whose updated column is (numerically) zero below the diagonal (the reference's tau = +inf case) or whose
// column fails the reference's rank test (factor.rs:52-64, evaluated from R): nothing of that panel has been written
// at that point, every earlier reflector has been applied to everything right of it, and geqrf_dev continues with the
// classic path on the remaining submatrix.  fp64 input (end of round 6) runs the same factorization with fp64 Gram sums: those are
// NOT exact, R~ is good to ~cond(panel)^2 eps64, so its guard keeps well-conditioned panels only (TqLim<double>::cond_max) and the
// classic path takes every other one.
#include <atomic>
#include <limits>

#include "common.h"
#include "mfma.h"

namespace fh {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TQ_PW = 64;   // panel width
constexpr int TQ_LP = 68;   // LDS pitch (floats) of one staged column of a 64-row chunk: 16-byte aligned, quad slots rotate
constexpr int TQ_TS = 192;  // widest strip of trailing columns per launch (LDS: 256 staged columns)
constexpr int TQ_NB = 512;  // workgroups (= partial sums) of a Gram launch: two per CU
constexpr int TQ_DP = 65;   // pitch of the fp64 64 x 64 matrices in LDS
constexpr double TQ_COND_MAX = 64.0 * 512.0; // |R D|_F |(R D)^-1|_F of the equilibrated panel (>= 64 for any panel): cond_2 below ~512
constexpr double TQ_TAIL_MIN = 1e-9;	     // 1 - |head| / |column| below this: the tail is numerically zero
// Per scalar type: the reference's epsilon (rank test), the condition bound of a panel and the range of column scales.
// fp32 data: the Gram sums are EXACT products accumulated in fp64, so R~ is good to cond^2 2^-53 -- far below fp32 rounding.
// fp64 data: the Gram sums carry fp64 rounding themselves, R~ and everything derived from it is good to ~cond^2 eps64: the
// one-pass path keeps panels whose equilibrated condition number is a small constant (|R D|_F |(R D)^-1|_F <= 128: cond_2 below
// ~8 for a graded spectrum; Gaussian and other well-conditioned tall panels) and hands everything else to the classic path.
template <typename T> struct TqLim;
template <> struct TqLim<float> {
	static constexpr double eps = 1.1920928955078125e-07;
	static constexpr double cond_max = TQ_COND_MAX;
	static constexpr double sq_lo = 1e-24, sq_hi = 1e24; // mean square of a column
};
template <> struct TqLim<double> {
	static constexpr double eps = 2.220446049250313e-16;
	static constexpr double cond_max = 64.0 * 2.0;
	static constexpr double sq_lo = 1e-200, sq_hi = 1e200;
};
enum { TQ_OK = 0, TQ_FAIL_CHOL = 1, TQ_FAIL_TAIL = 2, TQ_FAIL_RANK = 3, TQ_FAIL_COND = 4, TQ_FAIL_RANGE = 5 };

// Status word 0 of a factorization: 0, or 1 + the number of columns completed when a panel was rejected.  The kernels of
// the steps before the rejected panel still run (some of them beside the panel kernel that rejects), all later ones
// return at once: `c0` is the first column of the panel a launch belongs to.
static __device__ __forceinline__ void tq_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
static __device__ __forceinline__ bool tq_skip(const int *stat, int c0)
{
	const int s = *reinterpret_cast<const volatile int *>(stat);
	return s != 0 && c0 >= s - 1;
}

// ------------------------------------------------------------------------------------------------
// gram
// ------------------------------------------------------------------------------------------------
struct TqGramArgs {
	const float *P; // A[r0, c0]
	const float *X; // A[r0, cx]
	long ld;
	int rows, w, t, tp; // rows from r0 down, panel width, trailing columns of this launch, t rounded up to 32
	int nchunks;
	int want_g, want_sq;
	double *Gp; // [grid][64 * 64]
	float *Cp;  // [grid][64 * tp]
	float *Sp;  // [grid][256] per-column sums of squares of the staged columns (range guard of the first launch)
	const int *stat;
	int c0; // first column of the panel (tq_skip)
	float *A1s; // want_g: the panel's top 64 x 64 block, column major, for the panel kernel (see there)
};

template <bool VEC> __global__ __launch_bounds__(256, 2) void tq_gram_kernel(const TqGramArgs a)
{
	__shared__ float sm[(TQ_PW + TQ_TS) * TQ_LP];
	if (tq_skip(a.stat, a.c0))
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int quad = tid & 15, cg = tid >> 4;
	const int ncol = TQ_PW + a.tp;
	const int ntile = 2 * (a.tp >> 5);
	f64x4 gacc[3];
	f32x16 cacc[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
		gacc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int i = 0; i < 3; ++i)
#pragma unroll
		for (int r = 0; r < 16; ++r)
			cacc[i][r] = 0.f;
	float sq[16];
#pragma unroll
	for (int i = 0; i < 16; ++i)
		sq[i] = 0.f;
	f32x4 st[16];
	auto load_chunk = [&](int ch) {
		const int rbase = ch * 64 + quad * 4;
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			f32x4 v = {0.f, 0.f, 0.f, 0.f};
			const int c = i * 16 + cg;
			if (i * 16 < ncol) {
				const bool isp = c < TQ_PW;
				const int cc = isp ? c : c - TQ_PW;
				const bool colok = isp ? cc < a.w : cc < a.t;
				if (colok && rbase < a.rows) {
					const float *src = (isp ? a.P : a.X) + (long) cc * a.ld + rbase;
					if (VEC && rbase + 3 < a.rows) {
						v = *reinterpret_cast<const f32x4 *>(src);
					} else {
#pragma unroll
						for (int e = 0; e < 4; ++e)
							if (rbase + e < a.rows)
								v[e] = src[e];
					}
				}
			}
			st[i] = v;
		}
	};
	int ch = blockIdx.x;
	if (ch < a.nchunks)
		load_chunk(ch);
	for (; ch < a.nchunks; ch += gridDim.x) {
		__syncthreads(); // the previous chunk has been consumed
		if (ch == 0 && a.want_g) {
#pragma unroll
			for (int i = 0; i < 4; ++i)
				*reinterpret_cast<f32x4 *>(a.A1s + (i * 16 + cg) * 64 + quad * 4) = st[i];
		}
#pragma unroll
		for (int i = 0; i < 16; ++i)
			if (i * 16 < ncol) {
				*reinterpret_cast<f32x4 *>(&sm[(i * 16 + cg) * TQ_LP + quad * 4]) = st[i];
				if (a.want_sq)
					sq[i] += st[i][0] * st[i][0] + st[i][1] * st[i][1] + st[i][2] * st[i][2] + st[i][3] * st[i][3];
			}
		__syncthreads();
		if (ch + (int) gridDim.x < a.nchunks)
			load_chunk(ch + gridDim.x); // in flight during the products
		if (a.want_g) {
			// the 10 lower 16 x 16 tiles of G (the panel kernel reads the lower triangle only), three per wavefront:
			// lane: A[i = l & 15][k = l >> 4], four k-slices per 16-byte read
			const int t0 = wv == 0 ? 0x30 : (wv == 1 ? 0x33 : (wv == 2 ? 0x22 : 0x00)); // (ia << 4) | ib
			const int t1 = wv == 0 ? 0x31 : (wv == 1 ? 0x20 : (wv == 2 ? 0x10 : -1));
			const int t2 = wv == 0 ? 0x32 : (wv == 1 ? 0x21 : (wv == 2 ? 0x11 : -1));
#pragma unroll
			for (int s = 0; s < 4; ++s) {
				const int roff = 16 * s + 4 * (lane >> 4);
#pragma unroll
				for (int u = 0; u < 3; ++u) {
					const int tt = u == 0 ? t0 : (u == 1 ? t1 : t2);
					if (tt >= 0) { // wave uniform
						const f32x4 av = *reinterpret_cast<const f32x4 *>(&sm[(16 * (tt >> 4) + (lane & 15)) * TQ_LP + roff]);
						const f32x4 bv = *reinterpret_cast<const f32x4 *>(&sm[(16 * (tt & 15) + (lane & 15)) * TQ_LP + roff]);
#pragma unroll
						for (int q = 0; q < 4; ++q)
							gacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) av[q], (double) bv[q], gacc[u], 0, 0, 0);
					}
				}
			}
		}
		if (ntile > 0) {
			// 32 x 32 tiles of C: tile tl = wv + 4 u: panel half ia = tl & 1 = wv & 1, trailing 32-block ib = tl >> 1
			const int ia = wv & 1;
#pragma unroll
			for (int s = 0; s < 8; ++s) {
				const int roff = 8 * s + 4 * (lane >> 5);
				const f32x4 av = *reinterpret_cast<const f32x4 *>(&sm[(32 * ia + (lane & 31)) * TQ_LP + roff]);
#pragma unroll
				for (int u = 0; u < 3; ++u) {
					const int tl = wv + 4 * u;
					if (tl < ntile) {
						const int ib = tl >> 1;
						const f32x4 bv =
							*reinterpret_cast<const f32x4 *>(&sm[(TQ_PW + 32 * ib + (lane & 31)) * TQ_LP + roff]);
#pragma unroll
						for (int q = 0; q < 4; ++q)
							cacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], cacc[u], 0, 0, 0);
					}
				}
			}
		}
	}
	const long blk = blockIdx.x;
	if (a.want_g) {
		// f64 16x16x4 result map: col = lane & 15, row = (lane >> 4) + 4 * reg; tiles above the diagonal are never written
		const int t0 = wv == 0 ? 0x30 : (wv == 1 ? 0x33 : (wv == 2 ? 0x22 : 0x00));
		const int t1 = wv == 0 ? 0x31 : (wv == 1 ? 0x20 : (wv == 2 ? 0x10 : -1));
		const int t2 = wv == 0 ? 0x32 : (wv == 1 ? 0x21 : (wv == 2 ? 0x11 : -1));
#pragma unroll
		for (int u = 0; u < 3; ++u) {
			const int tt = u == 0 ? t0 : (u == 1 ? t1 : t2);
			if (tt >= 0) {
#pragma unroll
				for (int r = 0; r < 4; ++r)
					a.Gp[blk * 4096 + (16 * (tt >> 4) + (lane >> 4) + 4 * r) * 64 + 16 * (tt & 15) + (lane & 15)] = gacc[u][r];
			}
		}
	}
#pragma unroll
	for (int u = 0; u < 3; ++u) {
		const int tl = wv + 4 * u;
		if (tl < ntile) {
			const int ia = tl & 1, ib = tl >> 1;
			// f32 32x32x2 result map: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
				a.Cp[blk * 64 * a.tp + (long) (32 * ia + i) * a.tp + 32 * ib + (lane & 31)] = cacc[u][r];
			}
		}
	}
	if (a.want_sq) {
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			float v = sq[i];
			v += __shfl_xor(v, 1);
			v += __shfl_xor(v, 2);
			v += __shfl_xor(v, 4);
			v += __shfl_xor(v, 8);
			if (quad == 0)
				a.Sp[blk * 256 + i * 16 + cg] = v;
		}
	}
}

// Sums of the per-workgroup partials in a FIXED order, two levels: workgroup (x, g) adds the partials g, g + TQ_NG, ... of
// 256 entries into slice g of the output; the consumers (panel / y kernels) add the TQ_NG slices, again in a fixed order.
// One level (every entry summed over 512 partials by one thread) took 40-120 us per launch: 64 workgroups, 512 dependent
// strided loads each.
constexpr int TQ_NG = 8;
template <typename TC> __global__ __launch_bounds__(256) void tq_reduce_kernel(const double *Gp, const TC *Cp, const TC *Sp, int nb, int tp, int want_g,
							 int want_sq, double *G, double *C, int ldc, int coff, double *S, const int *stat, int c0,
							 double *Gf, int *cnt)
{
	__shared__ int s_last;
	if (tq_skip(stat, c0))
		return;
	const int e = blockIdx.x * 256 + threadIdx.x;
	const int g = blockIdx.y;
	const int ng = want_g ? 4096 : 0, nc = 64 * tp, ns = want_sq ? 256 : 0;
	if (blockIdx.x * 256 < ng) { // (4096 = 16 x 256: a workgroup is all G or not at all)
		// four independent sums (fixed assignment of the partials to them): eight loads in flight instead of two -- the loop is
		// a chain of memory round trips
		double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
		int b = g;
		for (; b + 3 * TQ_NG < nb; b += 4 * TQ_NG) {
			s0 += Gp[(long) b * 4096 + e];
			s1 += Gp[(long) (b + TQ_NG) * 4096 + e];
			s2 += Gp[(long) (b + 2 * TQ_NG) * 4096 + e];
			s3 += Gp[(long) (b + 3 * TQ_NG) * 4096 + e];
		}
		for (; b < nb; b += TQ_NG)
			s0 += Gp[(long) b * 4096 + e];
		G[(long) g * 4096 + e] = (s0 + s1) + (s2 + s3);
		// The slices of G are added up here as well, by whichever of the TQ_NG workgroups of these 256 entries finishes last
		// (fixed order of the slices): the panel kernel -- ONE workgroup -- then reads 32 KB instead of 256 KB, which took
		// it 35 000 cycles.  The counters return to zero by themselves.
		// (the barrier waits for every wavefront's stores; ONE release fence behind it publishes them all -- a fence per
		// thread made this kernel 19 -> 33 us)
		__syncthreads();
		if (threadIdx.x == 0) {
			__threadfence();
			const int old = atomicAdd(&cnt[blockIdx.x], 1);
			s_last = old == TQ_NG - 1;
			if (s_last)
				cnt[blockIdx.x] = 0;
		}
		__syncthreads();
		if (s_last) {
			__threadfence();
			double sum = 0.0;
			for (int q = 0; q < TQ_NG; ++q)
				sum += __builtin_nontemporal_load(&G[(long) q * 4096 + e]);
			Gf[e] = sum;
		}
		return;
	}
	if (e < ng) {
		// four independent sums (fixed assignment of the partials to them): eight loads in flight instead of two -- the loop is
		// a chain of memory round trips
		double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
		int b = g;
		for (; b + 3 * TQ_NG < nb; b += 4 * TQ_NG) {
			s0 += Gp[(long) b * 4096 + e];
			s1 += Gp[(long) (b + TQ_NG) * 4096 + e];
			s2 += Gp[(long) (b + 2 * TQ_NG) * 4096 + e];
			s3 += Gp[(long) (b + 3 * TQ_NG) * 4096 + e];
		}
		for (; b < nb; b += TQ_NG)
			s0 += Gp[(long) b * 4096 + e];
		G[(long) g * 4096 + e] = (s0 + s1) + (s2 + s3);
	} else if (e < ng + nc) {
		const int idx = e - ng;
		double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
		int b = g;
		for (; b + 3 * TQ_NG < nb; b += 4 * TQ_NG) {
			s0 += (double) Cp[(long) b * nc + idx];
			s1 += (double) Cp[(long) (b + TQ_NG) * nc + idx];
			s2 += (double) Cp[(long) (b + 2 * TQ_NG) * nc + idx];
			s3 += (double) Cp[(long) (b + 3 * TQ_NG) * nc + idx];
		}
		for (; b < nb; b += TQ_NG)
			s0 += (double) Cp[(long) b * nc + idx];
		const int arow = idx / tp, bcol = idx - arow * tp;
		C[((long) g * 64 + arow) * ldc + coff + bcol] = (s0 + s1) + (s2 + s3);
	} else if (e < ng + nc + ns) {
		const int idx = e - ng - nc;
		double s0 = 0;
		for (int b = g; b < nb; b += TQ_NG)
			s0 += (double) Sp[(long) b * 256 + idx];
		S[(long) g * 256 + idx] = s0;
	}
}

// ------------------------------------------------------------------------------------------------
// panel: everything 64 x 64, fp64, one workgroup of 256 threads (four wavefronts), blocked by 16 columns:
//   A1. Cholesky G = L L^T (R~ = L^T): diagonal block + the rows below it in wavefront 0 (tq_chol16, tq_subst16, which also
//       yields the diagonal block of L^-1 in its spare lanes), trailing update on the fp64 matrix cores;
//   A2. the rest of R~^-1 = L^-T block diagonal by block diagonal (tq_trinv_levels);   A3. Q1~ = A1 R~^-1 (products);
//   B1. the sign-choosing LU of I - Q1~ S = V1 U on its linear part W (column j of I - W S is e_j - s_j W_j): tq_lu16 on the
//       64 x 16 block column, U formed as soon as the block's signs are known, the 16 rows of U right of the block and the
//       diagonal block of V1^-1 by substitution, the Schur complement on the matrix cores; wavefront 1 inverts the
//       diagonal block of U one step behind;
//   B2. the rest of U^-1 and V1^-1 (tq_trinv_levels);   then the reference's rank test, the condition guard, the outputs.
// History (profiles/r03_qr_panel_phases.txt): barrier-separated loops over LDS-resident matrices: 314 us per panel (1.25 of
// the 3.4 ms of a 5e5 x 256 factorization at the time); every row in registers, one wavefront per kind of row, one workgroup
// barrier per 4 columns: 146 us; this version ~110 us.
// ------------------------------------------------------------------------------------------------
template <typename T> struct TqPanelArgs {
	T *A;
	long ld;
	int m, r0, c0, w, n;
	const double *G;   // the Gram matrix (sum of the TQ_NG slices), row major 64 x 64 (w x w valid, lower 16 x 16 tiles)
	const double *S;   // TQ_NG slices of the column squares of the first launch: [0, 64) panel, [64, ..) trailing
	int check_range, range_cols;
	double *abv;	   // per global column: sum of squares of the R entries above the current block row
	double *N1, *N3; // out: R^-T, V1^-1 (row major 64 x 64); with M they give Y = -M V1^-1 (R^-T C - X_top)
	T *Mn;	   // out: M = -(U R)^-1, row major 64 x 64
	const T *A1s;  // the panel's top block before the factorization, column major 64 x 64 (written by the Gram kernel)
	T *top;	   // out: the panel's top block (R on and above the diagonal, V1 below), row major 64 x 64 -- NOT written
			   // into A here: the Gram launch of this panel's trailing columns may still be reading those rows
	double *Md, *Td;   // out: M and T of this panel in fp64 (cross-panel blocks of T)
	T *H;
	long hrs, hcs;
	int bs;
	T *taus;
	int *stat;
	long long *dbg; // phase stamps (timing build only)
};

// 1 / a and 1 / sqrt(a) in fp64 from the hardware estimates and two Newton steps (the IEEE division / square-root
// sequences are ~40 dependent instructions each, on the critical path of every elimination step)
static __device__ __forceinline__ double tq_rcp(double a)
{
#ifdef TQ_EXACT_DIV
	return 1.0 / a;
#endif
	double r = __builtin_amdgcn_rcp(a);
	r = __builtin_fma(__builtin_fma(-a, r, 1.0), r, r);
	r = __builtin_fma(__builtin_fma(-a, r, 1.0), r, r);
	return r;
}
static __device__ __forceinline__ double tq_rsq(double a)
{
#ifdef TQ_EXACT_DIV
	return 1.0 / sqrt(a);
#endif
	double r = __builtin_amdgcn_rsq(a);
	r = __builtin_fma(__builtin_fma(-0.5 * a * r, r, 0.5), r, r);
	r = __builtin_fma(__builtin_fma(-0.5 * a * r, r, 0.5), r, r);
	return r;
}

static __device__ __forceinline__ double tq_rl(double v, int l)
{
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
	return __hiloint2double(hi, lo);
}

// The small-matrix work of tq_panel_kernel is BLOCKED by 16 columns: only the 16 x 16 diagonal blocks are eliminated column
// by column (inside ONE wavefront, rows in lanes, the 16 columns of the block in registers, pivots and pivot rows through
// v_readlane); everything else -- the blocks below / right of a diagonal block (a triangular substitution per lane), the
// trailing updates and the three triangular inverses (16 x 16 x 16 products on the fp64 matrix cores) -- has no per-column
// synchronisation at all.  The first version eliminated all 64 columns one after the other with every row in registers
// (one wavefront per kind of row, multipliers through LDS): 1 400 (Cholesky) and 2 750 (LU) cycles per column, 270 000 of
// the kernel's 470 000 cycles (profiles/r03_qr_panel_phases.txt).
// What was measured on the way (same file):
//   * a write by ONE lane followed by a wave-uniform read of the same LDS word needs a fence + wave barrier in between --
//     without it the read was hoisted above the masked store;
//   * code that runs once costs ~3.5 cycles per byte (instruction fetch, one cache line per L2 round trip): the kernel is
//     ONE workgroup that starts cold every launch, so unrolled bodies are kept to what is re-used by the four block steps.
static __device__ __forceinline__ void tq_lds_order()
{
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

// A 64 x 64 fp64 matrix in LDS seen through strides (a transposed view swaps them) and a structure mask in LOGICAL
// coordinates: 0 as stored, 1 lower incl. diagonal, 2 unit lower (the stored strictly lower part, ones on the diagonal),
// 3 upper incl. diagonal, 4 unit upper; rsc (optional): row r is scaled by rsc[r].
struct TqMat {
	const double *p;
	int rs, cs, mode;
	const double *rsc;
};
static __device__ __forceinline__ double tq_get(const TqMat &M, int r, int c)
{
	double v = M.p[r * M.rs + c * M.cs];
	if (M.mode == 1)
		v = c <= r ? v : 0.0;
	else if (M.mode == 2)
		v = c < r ? v : (c == r ? 1.0 : 0.0);
	else if (M.mode == 3)
		v = r <= c ? v : 0.0;
	else if (M.mode == 4)
		v = r < c ? v : (c == r ? 1.0 : 0.0);
	if (M.rsc)
		v *= M.rsc[r];
	return v;
}
// acc += A(tile ti, tile kt) * B(tile kt, tile tj); acc[q]: row (lane >> 4) + 4 q, column lane & 15 of the 16 x 16 tile
static __device__ __forceinline__ void tq_tile_mac(f64x4 &acc, const TqMat &A, int ti, const TqMat &B, int tj, int kt, int lane)
{
#pragma unroll
	for (int s4 = 0; s4 < 4; ++s4) {
		const int k = 16 * kt + 4 * s4 + (lane >> 4);
		const double av = tq_get(A, 16 * ti + (lane & 15), k);
		const double bv = tq_get(B, k, 16 * tj + (lane & 15));
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
	}
}

// The three column-by-column routines below work on FOUR columns per pass of a loop and then rotate the 16 registers by
// four positions, so that the columns in hand sit at the static positions 0 .. 3: one loop body of a quarter of the fully
// unrolled size (6 KB each, and the kernel runs at the speed of its instruction fetch) at nearly its speed (rotating by
// one position per column measured 2 000 cycles per column against 800).  In pass b position k holds column 4 b + k
// (mod 16); the positions with 4 b + k >= 16 are finished columns.
static __device__ __forceinline__ void tq_rot16(double (&x)[16])
{
	double t[4];
#pragma unroll
	for (int k = 0; k < 4; ++k)
		t[k] = x[k];
#pragma unroll
	for (int k = 0; k < 12; ++k)
		x[k] = x[k + 4];
#pragma unroll
	for (int k = 0; k < 4; ++k)
		x[12 + k] = t[k];
}

// Forward substitution with a 16 x 16 lower triangular block T (T[i][l] at T + i * trs + l * tcs, the same for every lane
// of a group), one right-hand side per lane in z:  z <- T^-1 z.  dinv: reciprocals of the diagonal, used by the lanes
// with `scaled` (the others have a unit diagonal).
// UNR = 4 (rotation by four) where the call is repeated per block step, 1 (a quarter of the code) where it runs once.
template <int UNR>
static __device__ __forceinline__ void tq_subst16(double (&z)[16], const double *T, int trs, int tcs, const double *dinv, bool scaled)
{
	if (UNR == 1) {
#pragma unroll 1
		for (int l = 0; l < 16; ++l) {
			const double dv = dinv[l];
			z[0] *= scaled ? dv : 1.0;
			const double *col = T + l * tcs + l * trs; // T[l + k][l] at col[k * trs]
#pragma unroll
			for (int k = 1; k < 16; ++k) {
				const double t = l + k < 16 ? col[k * trs] : 0.0; // wave uniform
				z[k] = __builtin_fma(-t, z[0], z[k]);
			}
			const double t0 = z[0];
#pragma unroll
			for (int k = 0; k < 15; ++k)
				z[k] = z[k + 1];
			z[15] = t0;
		}
		return;
	}
#pragma unroll 1
	for (int b = 0; b < 4; ++b) {
#pragma unroll
		for (int jj = 0; jj < 4; ++jj) {
			const int l = 4 * b + jj;
			const double dv = dinv[l];
			z[jj] *= scaled ? dv : 1.0;
			const double *col = T + l * tcs + (4 * b) * trs; // T[4 b + k][l] at col[k * trs]
			// all the reads first, unconditionally (beyond the block they land in the next rows of the LDS arrays and are
			// discarded): guarded one by one they were issued one by one, a full LDS latency each
			double t[16];
#pragma unroll
			for (int k = jj + 1; k < 16; ++k)
				t[k] = col[k * trs];
#pragma unroll
			for (int k = jj + 1; k < 16; ++k) {
				const double tk = 4 * b + k < 16 ? t[k] : 0.0; // wave uniform
				z[k] = __builtin_fma(-tk, z[jj], z[k]);
			}
		}
		tq_rot16(z);
	}
}

// Cholesky of the 16 x 16 block D (row i in lane i & 15, lanes >= 16 repeat the rows): x <- the lower factor, zeros above
// the diagonal; dinv16[J] <- 1 / L[J][J].  Returns true if a pivot is not positive (wave uniform).
static __device__ __forceinline__ bool tq_chol16(double (&x)[16], int lane, double *dinv16)
{
	const int i = lane & 15;
	bool bad = false;
#pragma unroll 1
	for (int b = 0; b < 4; ++b) {
#pragma unroll
		for (int jj = 0; jj < 4; ++jj) {
			const int J = 4 * b + jj;
			const double d = tq_rl(x[jj], J);
			bad = bad || !(d > 0.0) || !(d < 1e300);
			const double rinv = tq_rsq(d);
			const double a = x[jj] * rinv; // lane i >= J: L[i][J]
			x[jj] = i >= J ? a : 0.0;
			if (lane == J)
				dinv16[J] = rinv;
			// L[4 b + k][J] from lane (4 b + k) mod 16: for a finished column that lane is < J and holds the zero written above
#pragma unroll
			for (int k = jj + 1; k < 16; ++k)
				x[k] = __builtin_fma(-a, tq_rl(x[jj], (4 * b + k) & 15), x[k]);
		}
		tq_rot16(x);
	}
	return bad;
}

// The sign-choosing elimination (I - Q1~ S = V1 U on its linear part W, column j of I - W S is e_j - s_j W_j) of the 16
// columns c0 .. c0 + 15 of W, row r in lane r, the 16 entries of the row in x: afterwards x holds the multipliers V1[r][c]
// below the diagonal and the raw rows of U (U[j][c] = delta - s_c W[j][c] once every sign is known) on and above it.
// Returns true if the tail of a column is numerically zero (wave uniform).
static __device__ __forceinline__ bool tq_lu16(double (&x)[16], int r, int c0, int w, double *sgn, double *pinvs)
{
	// (fully unrolled: with the rotation scheme every column updated all 15 other positions, finished ones with a zero
	// factor selected on the scalar side -- 19 600 cycles per call against 9 700; the 3 KB of extra code cost less)
	bool bad = false;
#pragma unroll
	for (int J = 0; J < 16; ++J) {
		const int gJ = c0 + J;
		const double alpha = tq_rl(x[J], gJ);
		bad = bad || (gJ < w && !(1.0 - fabs(alpha) >= TQ_TAIL_MIN));
		const double sj = alpha >= 0.0 ? -1.0 : 1.0;
		const double pinv = tq_rcp(1.0 + fabs(alpha));
		const double mult = r > gJ ? -sj * x[J] * pinv : 0.0;
		if (r > gJ)
			x[J] = mult; // V1[r][gJ]
		if (r == gJ) {
			sgn[gJ] = sj;
			pinvs[gJ] = pinv;
		}
#pragma unroll
		for (int k = J + 1; k < 16; ++k)
			x[k] = __builtin_fma(-mult, tq_rl(x[k], gJ), x[k]); // the pivot row from lane gJ
	}
	return bad;
}

// One matrix of tq_trinv_levels: T lower triangular (logical), X = T^-1 read back through `X` (logical lower), written
// through (out, ors, ocs): X[r][c] at out[r * ors + c * ocs].  The diagonal blocks of X are already there.
struct TqInvJob {
	TqMat T, X;
	double *out;
	int ors, ocs;
};
// Off-diagonal blocks of the inverses of `nm` lower triangular matrices, block diagonal by block diagonal:
// X(i, j) = -X(i, i) sum_{k = j}^{i - 1} T(i, k) X(k, j); one workgroup barrier per diagonal.
static __device__ __forceinline__ void tq_trinv_levels(const TqInvJob &job0, const TqInvJob &job1, int nm, double *Pt, int wv, int lane)
{
#pragma unroll 1
	for (int d = 1; d < 4; ++d) {
		const int per = 4 - d;
#pragma unroll 1
		for (int t = wv; t < nm * per; t += 4) {
			const bool second = t >= per;
			TqInvJob jb; // (a run-time index into an array of jobs would put them into scratch memory)
			jb.T.p = second ? job1.T.p : job0.T.p;
			jb.T.rs = second ? job1.T.rs : job0.T.rs;
			jb.T.cs = second ? job1.T.cs : job0.T.cs;
			jb.T.mode = second ? job1.T.mode : job0.T.mode;
			jb.X.p = second ? job1.X.p : job0.X.p;
			jb.X.rs = second ? job1.X.rs : job0.X.rs;
			jb.X.cs = second ? job1.X.cs : job0.X.cs;
			jb.X.mode = second ? job1.X.mode : job0.X.mode;
			jb.T.rsc = nullptr;
			jb.X.rsc = nullptr;
			jb.out = second ? job1.out : job0.out;
			jb.ors = second ? job1.ors : job0.ors;
			jb.ocs = second ? job1.ocs : job0.ocs;
			const int j = second ? t - per : t, i = j + d;
			f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
			for (int k = j; k < i; ++k)
				tq_tile_mac(acc, jb.T, i, jb.X, j, k, lane);
#pragma unroll
			for (int q = 0; q < 4; ++q)
				Pt[((lane >> 4) + 4 * q) * 17 + (lane & 15)] = acc[q];
			tq_lds_order();
			const TqMat Pm = {Pt, 17, 1, 0, nullptr};
			f64x4 acc2 = {0.0, 0.0, 0.0, 0.0};
			// Pm is a single tile: rows 16 kt + .. with kt = 0 -- shift X instead
			{
#pragma unroll
				for (int s4 = 0; s4 < 4; ++s4) {
					const int k = 4 * s4 + (lane >> 4);
					const double av = tq_get(jb.X, 16 * i + (lane & 15), 16 * i + k);
					const double bv = Pm.p[k * 17 + (lane & 15)];
					acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc2, 0, 0, 0);
				}
			}
#pragma unroll
			for (int q = 0; q < 4; ++q)
				jb.out[(16 * i + (lane >> 4) + 4 * q) * jb.ors + (16 * j + (lane & 15)) * jb.ocs] = -acc2[q];
			tq_lds_order(); // Pt is reused by this wavefront's next task
		}
		__syncthreads();
	}
}

#ifdef FH_TQ_TIMING
#define TQ_STAMP(i)                                                                                                      \
	do {                                                                                                             \
		if (threadIdx.x == 0)                                                                                    \
			a.dbg[i] = (long long) __builtin_readcyclecounter();                                             \
	} while (0)
#else
#define TQ_STAMP(i)                                                                                                      \
	do {                                                                                                             \
	} while (0)
#endif
constexpr int TQ_PT = 256;
template <typename T> __global__ __launch_bounds__(TQ_PT) void tq_panel_kernel(const TqPanelArgs<T> a)
{
	__shared__ double Lm[64 * TQ_DP]; // G, then L (lower Cholesky factor, R~ = L^T), later M
	__shared__ double Wm[64 * TQ_DP]; // A1, then Q1~, then [V1 strictly lower | U upper]
	__shared__ double Ri[64 * TQ_DP]; // R~^-1 (upper)
	__shared__ double UL[64 * TQ_DP]; // U^-1 (upper incl. diagonal) | V1^-1 (strictly lower, unit diagonal implied)
	__shared__ double sgn[64], dinv[64], pinvs[64];
	__shared__ double Pt[4 * 16 * 17]; // one scratch tile per wavefront
	__shared__ int s_fail;
	if (a.stat[0])
		return;
	const int tid = threadIdx.x, w = a.w;
	const int r = tid & 63;
	const int kind = __builtin_amdgcn_readfirstlane(tid >> 6); // wavefront index, as a scalar
	TQ_STAMP(0);
	if (tid == 0)
		s_fail = 0;
	auto fail = [&](int why) {
		if (tid == 0) {
			a.stat[1] = a.c0;
			a.stat[2] = why;
			__threadfence();
			*reinterpret_cast<volatile int *>(a.stat) = a.c0 + 1;
		}
	};
	if (a.check_range) {
		// fp32 products of the C sums underflow / overflow for columns far from unit scale: rms outside [1e-12, 1e12]
		const double lo = TqLim<T>::sq_lo * (double) (a.m - a.r0), hi = TqLim<T>::sq_hi * (double) (a.m - a.r0);
		bool bad = false;
		for (int c = tid; c < w; c += TQ_PT) { // the trailing columns: tq_y_kernel of this step
			double sq = 0.0;
			for (int g = 0; g < TQ_NG; ++g)
				sq += a.S[g * 256 + c];
			bad = bad || !(sq >= lo && sq <= hi);
		}
		__syncthreads();
		if (bad)
			s_fail = TQ_FAIL_RANGE;
		__syncthreads();
		if (s_fail) {
			fail(TQ_FAIL_RANGE);
			return;
		}
	}
	TQ_STAMP(12);
	// ---- G (the sum of its TQ_NG slices, identity beyond w) and A1 (zero beyond w) through LDS, coalesced; the loads of four
	//      entries (36 of them) are in flight together: one entry at a time this was 36 000 cycles of dependent round trips
#pragma unroll 1
	for (int e0 = tid; e0 < 4096; e0 += 4 * TQ_PT) {
		double gs[4];
		T av[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) {
			const int e = e0 + u * TQ_PT;
			const int i = e >> 6, j = e & 63;
			const bool in = i < w && j < w;
			const int el = i >= j ? e : j * 64 + i; // the Gram kernel writes the lower 16 x 16 tiles only
			gs[u] = in ? a.G[el] : 0.0;
			// the top block as the Gram kernel's first workgroup copied it: read from A it is 64 columns on 64 different
			// pages (2 MB apart at m = 5e5), and this single workgroup waited for every one of the address translations
			av[u] = in ? a.A1s[e] : (T) 0;
		}
#pragma unroll
		for (int u = 0; u < 4; ++u) {
			const int e = e0 + u * TQ_PT;
			const int i = e >> 6, j = e & 63;
			double g = gs[u];
			if (!(i < w && j < w))
				g = i == j ? 1.0 : 0.0;
			Lm[i * TQ_DP + j] = g;
			Wm[j * TQ_DP + i] = (double) av[u];
			Ri[i * TQ_DP + j] = 0.0; // the blocks below its diagonal are never written, and the products read all of it
		}
	}
	TQ_STAMP(13);
	__syncthreads();
	TQ_STAMP(14);
	TQ_STAMP(1);
	const int lane = tid & 63, wv = kind;
	double *Ptw = Pt + wv * (16 * 17); // this wavefront's scratch tile
	// ---- A1: Cholesky G = L L^T (R~ = L^T), 16 columns per step: diagonal block and the rows below it in wavefront 0,
	//      the trailing update on the matrix cores
#pragma unroll 1
	for (int jb = 0; jb < 4; ++jb) {
		if (jb < 4)
			TQ_STAMP(16 + 2 * jb);
		const int c0 = 16 * jb;
		if (wv == 0) {
			double x[16];
			const int i = lane & 15;
#pragma unroll
			for (int c = 0; c < 16; ++c)
				x[c] = Lm[(c0 + i) * TQ_DP + c0 + c];
			if (tq_chol16(x, lane, dinv + c0) && lane == 0)
				s_fail = TQ_FAIL_CHOL;
			if (lane < 16) {
#pragma unroll
				for (int c = 0; c < 16; ++c)
					Lm[(c0 + i) * TQ_DP + c0 + c] = x[c];
			}
			tq_lds_order();
			// rows below: x L_d^T = b, one row per lane (at most 48); lanes 48 .. 63: the columns of L_d^-1, i.e. the
			// diagonal block of R~^-1 = L^-T -- the same substitution on unit vectors
			const int row = c0 + 16 + lane;
			const bool inv = lane >= 48, act = row < 64;
			const int j = lane - 48;
			double z[16];
#pragma unroll
			for (int c = 0; c < 16; ++c)
				z[c] = inv ? (c == j ? 1.0 : 0.0) : Lm[(act ? row : 63) * TQ_DP + c0 + c];
			tq_subst16<4>(z, Lm + c0 * TQ_DP + c0, TQ_DP, 1, dinv + c0, true);
			if (inv) {
#pragma unroll
				for (int c = 0; c < 16; ++c)
					Ri[(c0 + j) * TQ_DP + c0 + c] = z[c]; // L_d^-1[c][j], zero for c < j
			} else if (act) {
#pragma unroll
				for (int c = 0; c < 16; ++c)
					Lm[row * TQ_DP + c0 + c] = z[c];
			}
		}
		__syncthreads();
		if (s_fail) {
			fail(s_fail);
			return;
		}
		if (jb < 4)
			TQ_STAMP(17 + 2 * jb);
		if (jb < 3) {
			// G(ti, tj) -= L(ti, jb) L(tj, jb)^T for jb < tj <= ti
			const TqMat La = {Lm, TQ_DP, 1, 0, nullptr}, Lt = {Lm, 1, TQ_DP, 0, nullptr};
			int t = 0;
#pragma unroll 1
			for (int ti = jb + 1; ti < 4; ++ti)
#pragma unroll 1
				for (int tj = jb + 1; tj <= ti; ++tj, ++t) {
					if ((t & 3) != wv)
						continue;
					f64x4 acc = {0.0, 0.0, 0.0, 0.0};
					tq_tile_mac(acc, La, ti, Lt, tj, jb, lane);
#pragma unroll
					for (int q = 0; q < 4; ++q)
						Lm[(16 * ti + (lane >> 4) + 4 * q) * TQ_DP + 16 * tj + (lane & 15)] -= acc[q];
				}
			__syncthreads();
		}
	}
	// ---- A2: the blocks of R~^-1 = L^-T above its diagonal blocks, on the matrix cores
	{
		TqInvJob job;
		job.T = TqMat{Lm, TQ_DP, 1, 1, nullptr};
		job.X = TqMat{Ri, 1, TQ_DP, 1, nullptr};
		job.out = Ri;
		job.ors = 1;
		job.ocs = TQ_DP;
		tq_trinv_levels(job, job, 1, Ptw, wv, lane);
	}
	// ---- A3: Q1~ = A1 R~^-1 in place (row block wv is read and written by wavefront wv only)
	{
		// output block (wv, tj) overwrites an input of the blocks right of it only: right to left
		const TqMat Am = {Wm, TQ_DP, 1, 0, nullptr}, Rm = {Ri, TQ_DP, 1, 3, nullptr};
#pragma unroll 1
		for (int tj = 3; tj >= 0; --tj) {
			f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
			for (int kt = 0; kt <= tj; ++kt)
				tq_tile_mac(acc, Am, wv, Rm, tj, kt, lane);
			tq_lds_order();
#pragma unroll
			for (int q = 0; q < 4; ++q)
				Wm[(16 * wv + (lane >> 4) + 4 * q) * TQ_DP + 16 * tj + (lane & 15)] = acc[q];
			tq_lds_order();
		}
	}
	__syncthreads();
	TQ_STAMP(2);
	// ---- B1: the sign-choosing LU of W, 16 columns per step
#pragma unroll 1
	for (int jb = 0; jb < 4; ++jb) {
		TQ_STAMP(24 + 2 * jb);
		const int c0 = 16 * jb;
		if (wv == 0) {
			double x[16];
#pragma unroll
			for (int c = 0; c < 16; ++c)
				x[c] = Wm[lane * TQ_DP + c0 + c];
			if (tq_lu16(x, lane, c0, w, sgn, pinvs) && lane == 0)
				s_fail = TQ_FAIL_TAIL;
			tq_lds_order();
			// the signs of these 16 columns are known: U[r][c] = delta - s_c W[r][c] for every row r <= c of the column block
			// (the rows above the diagonal block hold what the earlier steps left there; nothing reads them raw any more)
#pragma unroll
			for (int c = 0; c < 16; ++c) {
				const double sc = sgn[c0 + c];
				if (c0 + c >= lane)
					x[c] = (c0 + c == lane ? 1.0 : 0.0) - sc * x[c];
			}
#pragma unroll
			for (int c = 0; c < 16; ++c)
				Wm[lane * TQ_DP + c0 + c] = x[c];
			tq_lds_order();
			// One substitution call per step, the lanes doing different things with it:
			//   lanes < 48 - 16 jb: the 16 rows of U right of the block, V1_d u = w, one column per lane;
			//   lanes 48 .. 63: the diagonal block of V1^-1 (unit vectors as right-hand sides) -- the same triangle, so every
			//   read of it stays wave uniform;
			//   last step only, lanes 0 .. 15: the diagonal block of U^-1 through U_d^T, whose reciprocal diagonal is pinvs
			//   (U_jj = 1 + |alpha_j|).  The other diagonal blocks of U^-1 are wavefront 1's, one step behind (below).
			const int nU = 48 - c0;
			const bool isU12 = lane < nU, v1l = lane >= 48, u3 = jb == 3 && lane < 16;
			const int j = lane & 15;
			const int col = c0 + 16 + lane;
			double z[16];
#pragma unroll
			for (int i = 0; i < 16; ++i)
				z[i] = isU12 ? Wm[(c0 + i) * TQ_DP + col] : (i == j ? 1.0 : 0.0);
			tq_subst16<4>(z, Wm + c0 * TQ_DP + c0, u3 ? 1 : TQ_DP, u3 ? TQ_DP : 1, pinvs + c0, u3);
			if (isU12) {
#pragma unroll
				for (int i = 0; i < 16; ++i)
					Wm[(c0 + i) * TQ_DP + col] = z[i];
			} else if (v1l) {
#pragma unroll
				for (int i = 0; i < 16; ++i)
					if (i > j)
						UL[(c0 + i) * TQ_DP + c0 + j] = z[i]; // V1^-1[i][j]
			} else if (u3) {
#pragma unroll
				for (int i = 0; i < 16; ++i)
					if (i >= j)
						UL[(c0 + j) * TQ_DP + c0 + i] = z[i]; // U^-1[j][i] = (U^T)^-1[i][j]
			}
		} else if (wv == 1 && jb >= 1 && lane < 16) {
			// beside wavefront 0: the diagonal block jb - 1 of U^-1 (that block of U is final since the last barrier)
			const int d0 = c0 - 16;
			double z[16];
#pragma unroll
			for (int i = 0; i < 16; ++i)
				z[i] = i == lane ? 1.0 : 0.0;
			tq_subst16<4>(z, Wm + d0 * TQ_DP + d0, 1, TQ_DP, pinvs + d0, true);
#pragma unroll
			for (int i = 0; i < 16; ++i)
				if (i >= lane)
					UL[(d0 + lane) * TQ_DP + d0 + i] = z[i];
		}
		__syncthreads();
		if (s_fail) {
			fail(s_fail);
			return;
		}
		TQ_STAMP(25 + 2 * jb);
		if (jb < 3) {
			// W(ti, tj) -= V1(ti, jb) U(jb, tj) for ti, tj > jb
			const TqMat Wa = {Wm, TQ_DP, 1, 0, nullptr};
			int t = 0;
#pragma unroll 1
			for (int ti = jb + 1; ti < 4; ++ti)
#pragma unroll 1
				for (int tj = jb + 1; tj < 4; ++tj, ++t) {
					if ((t & 3) != wv)
						continue;
					f64x4 acc = {0.0, 0.0, 0.0, 0.0};
					tq_tile_mac(acc, Wa, ti, Wa, tj, jb, lane);
#pragma unroll
					for (int q = 0; q < 4; ++q)
						Wm[(16 * ti + (lane >> 4) + 4 * q) * TQ_DP + 16 * tj + (lane & 15)] -= acc[q];
				}
			__syncthreads();
		}
	}
	TQ_STAMP(3);
	// ---- B2: the blocks of U^-1 (upper part of UL) and V1^-1 (strictly lower part) off their diagonal blocks
	{
		TqInvJob jobs[2];
		jobs[0].T = TqMat{Wm, 1, TQ_DP, 1, nullptr}; // U^T
		jobs[0].X = TqMat{UL, 1, TQ_DP, 1, nullptr};
		jobs[0].out = UL;
		jobs[0].ors = 1;
		jobs[0].ocs = TQ_DP;
		jobs[1].T = TqMat{Wm, TQ_DP, 1, 2, nullptr}; // V1
		jobs[1].X = TqMat{UL, TQ_DP, 1, 2, nullptr};
		jobs[1].out = UL;
		jobs[1].ors = TQ_DP;
		jobs[1].ocs = 1;
		tq_trinv_levels(jobs[0], jobs[1], 2, Ptw, wv, lane);
	}
	TQ_STAMP(15);
#ifdef FH_TQ_TIMING
	{
		// debug build: residuals of the three inverses, max over the workgroup -> dbg[9..11] (as doubles)
		__shared__ double s_res[3];
		if (tid < 3)
			s_res[tid] = 0.0;
		__syncthreads();
		double r1 = 0.0, r2 = 0.0, r3 = 0.0;
		for (int e = tid; e < 4096; e += TQ_PT) {
			const int i = e >> 6, j = e & 63;
			double a1 = 0.0, a2 = 0.0, a3 = 0.0;
			for (int l = 0; l < 64; ++l) {
				const double v1 = i > l ? Wm[i * TQ_DP + l] : (i == l ? 1.0 : 0.0);    // V1[i][l]
				const double li = l > j ? UL[l * TQ_DP + j] : (l == j ? 1.0 : 0.0);   // V1^-1[l][j]
				a1 += v1 * li;
				const double u = l >= i ? Wm[i * TQ_DP + l] : 0.0;                     // U[i][l]
				const double ui = l <= j ? UL[l * TQ_DP + j] : 0.0;                    // U^-1[l][j]
				a2 += u * ui;
				const double rt = l >= i ? Lm[l * TQ_DP + i] : 0.0;                    // R~[i][l] = L[l][i]
				const double ri = l <= j ? Ri[l * TQ_DP + j] : 0.0;
				a3 += rt * ri;
			}
			const double d = i == j ? 1.0 : 0.0;
			r1 = fmax(r1, fabs(a1 - d));
			r2 = fmax(r2, fabs(a2 - d));
			r3 = fmax(r3, fabs(a3 - d));
		}
		for (int q = 0; q < TQ_PT; ++q) {
			if (tid == q) {
				s_res[0] = fmax(s_res[0], r1);
				s_res[1] = fmax(s_res[1], r2);
				s_res[2] = fmax(s_res[2], r3);
			}
			__syncthreads();
		}
		if (tid == 0) {
			a.dbg[9] = __double_as_longlong(s_res[0]);
			a.dbg[10] = __double_as_longlong(s_res[1]);
			a.dbg[11] = __double_as_longlong(s_res[2]);
		}
	}
#endif
	TQ_STAMP(4);
	// ---- the reference's rank test (wave 0), condition estimate (wave 1)
	if (tid < 64) {
		// factor.rs:52-64: |R_jj| > eps * 16 * (m - row) * hypot(|R_jj|, |R[0 .. j, j]|)
		const int j = tid;
		if (j < w) {
			double ab = a.abv[a.c0 + j];
			for (int l = 0; l < j; ++l)
				ab += Lm[j * TQ_DP + l] * Lm[j * TQ_DP + l];
			const double rjj = Lm[j * TQ_DP + j];
			const double full = sqrt(rjj * rjj + ab);
			const double thr = TqLim<T>::eps * 16.0 * (double) (a.m - a.c0 - j) * full;
			if (!(rjj > thr))
				atomicMax(&s_fail, (int) TQ_FAIL_RANK);
		}
	} else if (tid < 128) {
		// The estimate is taken on the EQUILIBRATED panel P D, D = diag(1 / |column|): its factor is R~ D (row ti of L scaled
		// to unit length, |R~ D|_F^2 = 64) and (R~ D)^-1 = D^-1 R~^-1.  What the one-pass path loses to rounding -- the
		// Cholesky factorization of G, V = P M, the trailing rows of R -- is invariant under column scaling, so a panel whose
		// columns merely differ in scale stays here; the unscaled estimate of round 3 sent it to the classic path.
		const int ti = tid - 64;
		double g2 = 0.0; // |column ti|^2 = G_ii = |row ti of L|^2
		for (int l = 0; l < 64; ++l)
			g2 += l <= ti ? Lm[ti * TQ_DP + l] * Lm[ti * TQ_DP + l] : 0.0;
		double f2 = 0.0;
		for (int l = 0; l < 64; ++l) {
			const double gl = __shfl(g2, l);
			f2 += l <= ti ? Ri[l * TQ_DP + ti] * Ri[l * TQ_DP + ti] * gl : 0.0;
		}
		for (int o = 32; o > 0; o >>= 1)
			f2 += __shfl_xor(f2, o);
		if (!(sqrt(64.0 * f2) <= TqLim<T>::cond_max))
			atomicMax(&s_fail, (int) TQ_FAIL_COND);
	}
	__syncthreads();
	if (s_fail) {
		fail(s_fail);
		return;
	}
	TQ_STAMP(5);
	// ---- outputs that read L: the top block of A (R = S R~ on and above the diagonal, V1 below), N1 = R^-T, N3 = V1^-1
	for (int e = tid; e < 4096; e += TQ_PT) {
		const int i = e >> 6, j = e & 63;
		a.top[e] = (T) (i <= j ? sgn[i] * Lm[j * TQ_DP + i] : Wm[i * TQ_DP + j]);
		// R^-1 = R~^-1 S  =>  N1[i][l] = R^-1[l][i] = Ri[l][i] * s_i  (Ri holds only its upper triangle)
		a.N1[e] = j <= i ? Ri[j * TQ_DP + i] * sgn[i] : 0.0;
		a.N3[e] = i == j ? 1.0 : (j < i ? UL[i * TQ_DP + j] : 0.0);
	}
	__syncthreads(); // all reads of L are done
	TQ_STAMP(6);
	// ---- M = -R~^-1 S U^-1 and T = triu(V1^T U^-1), both upper triangular, on the fp64 matrix cores: wavefront wv owns the
	//      block row wv (as scalar dot products of triangular length out of LDS they were 120 000 cycles of this kernel);
	//      one loop body for both products
	const bool big_bs = a.bs >= TQ_PW;
	const float bs_rcp = 1.0f / (float) a.bs;
	const int hrow0 = big_bs ? a.c0 % a.bs : 0; // row of H that holds T's row 0
#pragma unroll 1
	for (int pass = 0; pass < 2; ++pass) {
		TqMat Am, Bm;
		Am.p = pass ? Wm : Ri;
		Am.rs = pass ? 1 : TQ_DP;
		Am.cs = pass ? TQ_DP : 1;
		Am.mode = pass ? 4 : 3; // V1^T (unit upper) : R~^-1 (upper)
		Am.rsc = nullptr;
		Bm.p = UL;
		Bm.rs = TQ_DP;
		Bm.cs = 1;
		Bm.mode = 3;
		Bm.rsc = pass ? nullptr : sgn; // S U^-1
#pragma unroll 1
		for (int tj = 0; tj < 4; ++tj) {
			f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
			for (int kt = wv; kt <= tj; ++kt)
				tq_tile_mac(acc, Am, wv, Bm, tj, kt, lane);
#pragma unroll
			for (int q = 0; q < 4; ++q) {
				const int k = 16 * wv + (lane >> 4) + 4 * q, j = 16 * tj + (lane & 15);
				if (pass == 0) {
					const double mv = k <= j ? -acc[q] : 0.0;
					a.Mn[k * 64 + j] = (T) mv;
					a.Md[k * 64 + j] = mv;
				} else {
					const double tt = k <= j ? acc[q] : 0.0;
					if (k <= j && j < w) {
						// rows / columns k, j < 64 of a panel that starts at a multiple of 64; the block size of Q_coeff is a
						// multiple of 64 or divides it (tsqr_applicable): no integer division per entry
						const int kb = big_bs ? 0 : (int) (((float) k + 0.5f) * bs_rcp), jbk = big_bs ? 0 : (int) (((float) j + 0.5f) * bs_rcp);
						if (kb == jbk)
							a.H[(long) (hrow0 + k - kb * a.bs) * a.hrs + (long) (a.c0 + j) * a.hcs] = (T) tt;
						if (k == j)
							a.taus[a.c0 + j] = (T) tt;
					}
					a.Td[k * 64 + j] = tt;
				}
			}
		}
		if (pass == 0)
			TQ_STAMP(7);
	}
	TQ_STAMP(8);
}

// ------------------------------------------------------------------------------------------------
// y: 16 trailing columns per workgroup
// ------------------------------------------------------------------------------------------------
template <typename T> struct TqYArgs {
	T *A;
	long ld;
	int r0, cx, w, t;
	const double *C; // TQ_NG slices, each row major 64 x ldc
	int ldc;
	const double *N1, *N3, *Md; // R^-T, V1^-1, M = -(U R)^-1
	double *abv;
	T *Yn; // out: -Y, row major 64 x typ
	int typ;
	double *Z; // out: Z = -V1^-1 (D - X_top) = T^-H V^H X, row major 64 x ldz, column index = GLOBAL column
	int ldz;
	const T *top; // the panel's top block as the panel kernel left it (workgroup 0 stores it into A)
	int *stat;
	const double *Sr; // first step only (check_range): TQ_NG slices of the column squares, trailing columns at [64, 64 + range_cols)
	int check_range, range_cols, mrows;
};

// the panel's top block from its staging copy into A (once every reader of the original rows is done)
template <typename T> static __device__ __forceinline__ void tq_store_top(T *A, long ld, int r0, int c0, int w, const T *top, int tid)
{
	for (int e = tid; e < 4096; e += 256) {
		const int i = e >> 6, j = e & 63;
		if (i < w && j < w)
			A[(long) (c0 + j) * ld + r0 + i] = top[e];
	}
}
template <typename T> __global__ __launch_bounds__(256) void tq_top_kernel(T *A, long ld, int r0, int c0, int w, const T *top, const int *stat)
{
	if (tq_skip(stat, c0))
		return;
	tq_store_top(A, ld, r0, c0, w, top, threadIdx.x);
}

template <typename T> __global__ __launch_bounds__(256) void tq_y_kernel(const TqYArgs<T> a)
{
	__shared__ double n1[64 * TQ_DP], n3[64 * TQ_DP], mm[64 * TQ_DP];
	__shared__ double v[64 * 17], v2[64 * 17];
	__shared__ double sred[256];
	if (tq_skip(a.stat, a.r0))
		return;
	const int tid = threadIdx.x;
	if (a.check_range) {
		// fp32 products of the C sums underflow / overflow for columns far from unit scale: rms outside [1e-12, 1e12] (the
		// panel kernel checked its own columns).  Every workgroup evaluates the same sums; nothing has been written yet.
		const double lo = TqLim<T>::sq_lo * (double) a.mrows, hi = TqLim<T>::sq_hi * (double) a.mrows;
		int bad = 0;
		if (tid < a.range_cols) {
			double sq = 0.0;
			for (int g = 0; g < TQ_NG; ++g)
				sq += a.Sr[g * 256 + 64 + tid];
			bad = !(sq >= lo && sq <= hi);
		}
		if (__syncthreads_or(bad)) {
			if (blockIdx.x == 0 && tid == 0) {
				a.stat[1] = a.r0;
				a.stat[2] = TQ_FAIL_RANGE;
				__threadfence();
				*reinterpret_cast<volatile int *>(a.stat) = a.r0 + 1;
			}
			return;
		}
	}
	if (blockIdx.x == 0)
		tq_store_top(a.A, a.ld, a.r0, a.cx - a.w, a.w, a.top, tid);
	// (24 loads of a thread in flight per batch: one element per iteration was 16 dependent memory round trips)
#pragma unroll 1
	for (int e0 = tid; e0 < 4096; e0 += 8 * 256) {
		double t1[8], t3[8], tm[8];
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			t1[u] = a.N1[e0 + 256 * u];
			t3[u] = a.N3[e0 + 256 * u];
			tm[u] = a.Md[e0 + 256 * u];
		}
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			const int e = e0 + 256 * u;
			n1[(e >> 6) * TQ_DP + (e & 63)] = t1[u];
			n3[(e >> 6) * TQ_DP + (e & 63)] = t3[u];
			mm[(e >> 6) * TQ_DP + (e & 63)] = tm[u];
		}
	}
	// Three 64 x 64 x 16 products on the fp64 matrix cores (round 6; rounds 3-5 ran them as rolled dot-product loops over LDS, a chain of
	// dependent LDS round trips: 27 us per launch).  Wavefront wv owns rows 16 wv .. + 15 of a product: result map of v_mfma_f64_16x16x4:
	// column = lane & 15, row = (lane >> 4) + 4 reg.  The triangles are applied as masks on the A operand.
	const int lane = tid & 63, wv = tid >> 6;
	const int bl = lane & 15, b = blockIdx.x * 16 + bl;
	const bool colok = b < a.t;
	{
		const int ig = tid >> 4; // rows ig, ig + 16, ig + 32, ig + 48 of column tid & 15: all 32 loads of a thread in flight at once
		const int bb = blockIdx.x * 16 + (tid & 15);
		double cv[4][TQ_NG];
#pragma unroll
		for (int u = 0; u < 4; ++u)
#pragma unroll
			for (int g = 0; g < TQ_NG; ++g)
				cv[u][g] = bb < a.t ? a.C[((long) g * 64 + ig + 16 * u) * a.ldc + bb] : 0.0;
#pragma unroll
		for (int u = 0; u < 4; ++u) {
			double c = 0.0;
#pragma unroll
			for (int g = 0; g < TQ_NG; ++g)
				c += cv[u][g];
			v[(ig + 16 * u) * 17 + (tid & 15)] = c;
		}
	}
	__syncthreads();
	// acc = Am (rows 16 wv .., masked: lower / upper triangle incl. the diagonal) * Bv (64 x 16)
	auto mm16 = [&](const double *Am, const double *Bv, bool lower) {
		f64x4 acc = {0.0, 0.0, 0.0, 0.0};
		const int i = 16 * wv + (lane & 15);
#pragma unroll 4
		for (int k0 = 0; k0 < 64; k0 += 4) {
			const int l = k0 + (lane >> 4);
			double av = Am[i * TQ_DP + l];
			if (lower ? l > i : l < i)
				av = 0.0;
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bv[l * 17 + (lane & 15)], acc, 0, 0, 0);
		}
		return acc;
	};
	// D = R^-T C: the new top rows of X; E = D - X_top
	{
		const f64x4 acc = mm16(n1, v, true);
		double dsq = 0.0;
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int i = 16 * wv + (lane >> 4) + 4 * r;
			dsq += acc[r] * acc[r];
			T *xp = a.A + (long) (a.cx + b) * a.ld + a.r0 + i;
			double xt = 0.0;
			if (colok && i < a.w) {
				xt = (double) *xp;
				*xp = (T) acc[r];
			}
			v2[i * 17 + bl] = acc[r] - xt;
		}
		sred[tid] = dsq;
	}
	__syncthreads();
	// column norms of the R rows just produced (rank test of the later panels)
	if (tid < 16 && blockIdx.x * 16 + tid < a.t) {
		double s = 0.0;
		for (int g = 0; g < 16; ++g)
			s += sred[g * 16 + tid]; // (tid & 15 == column in every group of 16 threads)
		a.abv[a.cx + blockIdx.x * 16 + tid] += s;
	}
	// zn = V1^-1 (D - X_top) = -Z, then  -Y = M zn  (Y = R^-1 U^-1 V1^-1 (D - X_top), M = -(U R)^-1 upper triangular)
	{
		const f64x4 acc = mm16(n3, v2, true);
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int k = 16 * wv + (lane >> 4) + 4 * r;
			v[k * 17 + bl] = acc[r]; // (every read of the C sums in v is behind the barrier above)
			if (colok)
				a.Z[(long) k * a.ldz + a.cx + b] = -acc[r];
		}
	}
	__syncthreads();
	{
		const f64x4 acc = mm16(mm, v, false);
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int k = 16 * wv + (lane >> 4) + 4 * r;
			if (b < a.typ)
				a.Yn[(long) k * a.typ + b] = colok ? (T) acc[r] : (T) 0;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// V = P M over the panel rows below its top block (stored over them)
// ------------------------------------------------------------------------------------------------
struct TqFormVArgs {
	float *P; // A[r1, c0], r1 = first row below the top block
	long ld;
	int rows, w; // rows from r1 down
	const float *Mn;
	int nrb; // 128-row blocks
	const int *stat;
	int c0; // first column of the panel (tq_skip)
};

template <bool VEC> static __device__ __forceinline__ f32x4 tq_ld4(const float *col, int lam, int rows)
{
	f32x4 v = {0.f, 0.f, 0.f, 0.f};
	if (VEC) {
		const int r = 4 * lam;
		if (r + 3 < rows) {
			v = *reinterpret_cast<const f32x4 *>(col + r);
		} else {
#pragma unroll
			for (int e = 0; e < 4; ++e)
				if (r + e < rows)
					v[e] = col[r + e];
		}
	} else {
#pragma unroll
		for (int q = 0; q < 4; ++q)
			if (32 * q + lam < rows)
				v[q] = col[32 * q + lam];
	}
	return v;
}
template <bool VEC> static __device__ __forceinline__ void tq_st4(float *col, int lam, int rows, f32x4 v)
{
	if (VEC) {
		const int r = 4 * lam;
		if (r + 3 < rows) {
			*reinterpret_cast<f32x4 *>(col + r) = v;
		} else {
#pragma unroll
			for (int e = 0; e < 4; ++e)
				if (r + e < rows)
					col[r + e] = v[e];
		}
	} else {
#pragma unroll
		for (int q = 0; q < 4; ++q)
			if (32 * q + lam < rows)
				col[32 * q + lam] = v[q];
	}
}

// One wavefront owns 128 rows: its 128 x 64 block of the panel is loaded ONCE into registers (32 quads per lane: lane
// l & 31 holds rows 4 (l & 31) .. + 3 of column 2 i + (l >> 5) -- row slot q of the four interleaved 32-row tiles), then
// the two 32-column strips of V = P M are formed and stored over the panel rows the wave has in registers.
template <bool VEC> __global__ __launch_bounds__(256, 1) void tq_form_v_kernel(const TqFormVArgs a)
{
	__shared__ float Ms[64 * 64];
	if (tq_skip(a.stat, a.c0))
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	{
		// M (row major 64 x 64) as it is: 16 independent loads in flight per thread
		float v[16];
#pragma unroll
		for (int u = 0; u < 16; ++u)
			v[u] = a.Mn[u * 256 + tid];
#pragma unroll
		for (int u = 0; u < 16; ++u)
			Ms[u * 256 + tid] = v[u];
	}
	__syncthreads();
	const int lam = lane & 31, h = lane >> 5;
	const int nv = (a.w + 31) >> 5; // strips of V
	for (int rbi = blockIdx.x * 4 + wv; rbi < a.nrb; rbi += gridDim.x * 4) {
		// The row blocks are visited from the LAST one up, the Gram launches read from the first row down: each pass starts with what the
		// pass before it touched last, i.e. with what the memory-side cache (256 MB) still holds
		const int rb = a.nrb - 1 - rbi;
		const int rows = a.rows - rb * 128; // valid rows from the block's first row (may exceed 128)
		float *Pb = a.P + (long) rb * 128;
		f32x4 pr[32];
#pragma unroll
		for (int i = 0; i < 32; ++i) {
			const int kc = 2 * i + h;
			pr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
			if (kc < a.w)
				pr[i] = tq_ld4<VEC>(Pb + (long) kc * a.ld, lam, rows);
		}
#pragma unroll 1
		for (int sc = 0; sc < nv; ++sc) {
			const int nvalid = a.w - 32 * sc;
			float *dst = Pb + (long) (32 * sc) * a.ld;
			f32x16 acc[4];
#pragma unroll
			for (int r = 0; r < 16; ++r)
#pragma unroll
				for (int q = 0; q < 4; ++q)
					acc[q][r] = 0.f;
#pragma unroll
			for (int i = 0; i < 32; ++i) {
				const float a0 = Ms[(2 * i + h) * 64 + 32 * sc + lam];
#pragma unroll
				for (int q = 0; q < 4; ++q)
					acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, pr[i][q], acc[q], 0, 0, 0);
			}
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int j = (r & 3) + 8 * (r >> 2) + 4 * h;
				if (j < nvalid)
					tq_st4<VEC>(dst + (long) j * a.ld, lam, rows, f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]});
			}
		}
	}
}

// ------------------------------------------------------------------------------------------------
// update + Gram in ONE pass (round 6): panel k's block reflector applied to the next panel's columns N and / or a strip F of the columns
// behind them, V = P M, and -- from the UPDATED values, which never leave the CU in between -- the Gram products of panel k + 1:
// G' = N'^T N' (fp64 matrix cores) and C' = N'^T F' (fp32).  Rounds 3-5 wrote X' out and read it back for the Gram launch: 2.5 of the 7.5
// passes of a 5e5 x 256 factorization.  64-row chunks are staged through LDS as [P | N | F] (column major, quads of four consecutive rows);
//   update   a wavefront owns one 32-row half of the chunk and up to three 32-column tiles: D = X + P (-Y) on v_mfma_f32_32x32x2 with the
//            P operand from LDS and ITS -Y operand in registers for the whole launch (the tiles of a wavefront are the same in every
//            chunk); the result map of the instruction (lane = column, registers = four groups of four consecutive rows) goes back into
//            the chunk as 16-byte quads; V = P M the same way into its own 64 columns of LDS;
//   store    every thread writes the quads it staged (its own columns: 16-byte stores, 256 contiguous bytes per column and 16 lanes);
//   gram     the products of tq_gram_kernel on the updated chunk.
// Modes (driver): U1 = N updated, G' formed (the panel kernel of k + 1 starts behind it); U2 = N read only, F updated, C' formed, beside
// that panel kernel; V = P M rides on whichever of the two runs beside the panel kernel.
// ------------------------------------------------------------------------------------------------
struct TqFusedArgs {
	float *P;	// A[r1, c0]: panel k below its top block
	float *N;	// A[r1, c0 + w]: the next panel's columns
	float *F;	// A[r1, c0 + w + wn + fo]: a strip of the columns behind them
	long ld;
	int rows;	// m - r1
	int w, wn, ts;	// widths: panel (<= 64), next panel (<= 64, 0: none), strip (<= 128, 0: none)
	int upd_n;	// N is updated (else read only: the A operand of C')
	int do_v, want_g;
	const float *Yn; // -Y, row major 64 x typ, column = index inside the trailing block
	int typ, fo;	// fo: first column of F behind N
	const float *Mn; // M, row major 64 x 64
	double *Gp;	// [grid][64 * 64]
	float *Cp;	// [grid][64 * tp]
	int tp;		// ts rounded up to 32
	int nchunks;
	float *A1s;	// want_g: the next panel's (updated) top 64 x 64 block, column major, for the panel kernel
	long ldp;	// leading dimension of P (MODE 2 may read the panel from the copy)
	float *Pc;	// MODE 1 with do_v: if set, the RAW panel rows are saved here (leading dimension ldpc) for the U2 launches that follow
	long ldpc;
	const int *stat;
	int c0;
};

constexpr int TU_CF = 128;		      // widest strip F
// Barrier between LDS phases that leaves global memory operations in flight (__syncthreads() is a workgroup-scope fence as well)
// MODE 1 (U1): stages [P | N], updates N, forms G', V = P M if asked.  MODE 2 (U2): stages [P | N | F], updates F, forms C' = N^T F'.
// Two variants instead of one general kernel: each needs fewer than 256 registers and 52 / 70 KB of LDS, so TWO workgroups share a CU --
// twice the bytes in flight (one general workgroup per CU with one 64 KB chunk in flight ran at 1.2-1.6 TB/s: a chunk per memory round
// trip) and one workgroup's products behind the other's barriers.
template <bool VEC, int MODE> __global__ __launch_bounds__(MODE == 1 ? 256 : 512, MODE == 1 ? 2 : 4) void tq_fused_kernel(const TqFusedArgs a)
{
	constexpr int NTHR = MODE == 1 ? 256 : 512; // MODE 2: eight wavefronts, one tile of F and one of C' each
	constexpr int CGN = NTHR / 16;		    // columns staged per pass of the threads
	constexpr int NC = MODE == 1 ? 2 * TQ_PW : 2 * TQ_PW + TU_CF; // staged columns
	constexpr int NQ = NC / CGN;				       // quads per thread and chunk
	constexpr int NT = 1;					       // column tiles per wavefront
	__shared__ float sm[NC * TQ_LP];
	__shared__ float vs[MODE == 1 ? TQ_PW * TQ_LP : 4];
	if (tq_skip(a.stat, a.c0))
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int quad = tid & 15;
	int cg = tid >> 4; // (MODE 2: made opaque once per chunk, see the loop)
	const int lam = lane & 31, h = lane >> 5;
	const int rt = wv & 1, cp = wv >> 1; // this wavefront's 32-row half of a chunk, and the parity of its column tiles
	// ---- the wavefront's operands of the whole launch: -Y for its column tiles (MODE 1: tile cp of N; MODE 2: tile cp of F), M for its V tile
	float yreg[NT][32], mreg[MODE == 1 ? 32 : 1];
	bool act[NT];
#pragma unroll
	for (int u = 0; u < NT; ++u) {
		const int cl = 32 * cp; // first column of the tile inside N / F
		act[u] = MODE == 1 ? cl < a.wn : cl < a.ts;
		const bool cok = MODE == 1 ? cl + lam < a.wn : cl + lam < a.ts;
		const int yc = MODE == 1 ? cl + lam : a.wn + a.fo + cl + lam;
#pragma unroll
		for (int s2 = 0; s2 < 32; ++s2) {
			const int k = 2 * s2 + h;
			yreg[u][s2] = (act[u] && cok && k < a.w) ? a.Yn[(long) k * a.typ + yc] : 0.f;
		}
	}
	const bool vact = MODE == 1 && a.do_v && 32 * cp < a.w;
	if (MODE == 1) {
#pragma unroll
		for (int s2 = 0; s2 < 32; ++s2) {
			const int k = 2 * s2 + h;
			mreg[s2] = (vact && k < a.w && 32 * cp + lam < a.w) ? a.Mn[k * 64 + 32 * cp + lam] : 0.f;
		}
	}
	const int ntile = MODE == 2 ? 2 * (a.tp >> 5) : 0; // 32 x 32 tiles of C'
	f64x4 gacc[MODE == 1 ? 3 : 1];
	f32x16 cacc[1];
#pragma unroll
	for (int i = 0; i < (MODE == 1 ? 3 : 1); ++i)
		gacc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int r = 0; r < 16; ++r)
		cacc[0][r] = 0.f;
	// column c of the staged chunk: source pointer (nullptr: not staged) -- thread (quad, cg) stages the columns 16 i + cg
	auto col_ptr = [&](int c) -> float * {
		if (c < TQ_PW)
			return c < a.w ? a.P + (long) c * a.ldp : nullptr;
		if (c < 2 * TQ_PW)
			return c - TQ_PW < a.wn ? a.N + (long) (c - TQ_PW) * a.ld : nullptr;
		return c - 2 * TQ_PW < a.ts ? a.F + (long) (c - 2 * TQ_PW) * a.ld : nullptr;
	};
	f32x4 st[NQ];
	auto load_chunk = [&](int ch) {
		const int rbase = ch * 64 + quad * 4;
#pragma unroll
		for (int i = 0; i < NQ; ++i) {
			f32x4 v = {0.f, 0.f, 0.f, 0.f};
			const float *src = col_ptr(i * CGN + cg);
			if (src && rbase < a.rows) {
				src += rbase;
				if (VEC && rbase + 3 < a.rows) {
					v = *reinterpret_cast<const f32x4 *>(src);
				} else {
#pragma unroll
					for (int e = 0; e < 4; ++e)
						if (rbase + e < a.rows)
							v[e] = src[e];
				}
			}
			st[i] = v;
		}
	};
	auto store_quad = [&](float *dst, int rbase, f32x4 v) {
		if (rbase >= a.rows)
			return;
		dst += rbase;
		if (VEC && rbase + 3 < a.rows) {
			*reinterpret_cast<f32x4 *>(dst) = v;
		} else {
#pragma unroll
			for (int e = 0; e < 4; ++e)
				if (rbase + e < a.rows)
					dst[e] = v[e];
		}
	};
	constexpr int XC0 = MODE == 1 ? TQ_PW : 2 * TQ_PW; // first staged column of the updated block
	int ch = blockIdx.x;
	if (ch < a.nchunks)
		load_chunk(ch);
	for (; ch < a.nchunks; ch += gridDim.x) {
		// MODE 2 has 128 registers per wavefront; the compiler kept the loop-invariant column pointers of the loads and stores (12 64-bit
		// values per thread) and spilled 16 registers of the -Y operand for them -- and on gfx9 a scratch reload counts in the same
		// in-order counter as the global loads: every reload inside the products waited for the NEXT chunk's loads, which had just been
		// issued.  An opaque copy of the column group makes it recompute the pointers where they are used (114 registers, no spill:
		// U2 220 -> 200 us; in MODE 1, which has the registers, the same trick costs 18 us per launch and is not applied).
		if (MODE == 2)
			asm volatile("" : "+v"(cg));
		tq_lds_barrier(); // the previous chunk has been consumed
#pragma unroll
		for (int i = 0; i < NQ; ++i)
			*reinterpret_cast<f32x4 *>(&sm[(i * CGN + cg) * TQ_LP + quad * 4]) = st[i];
		tq_lds_barrier();
		if (MODE == 2)
			asm volatile("" : "+v"(cg));
		if (ch + (int) gridDim.x < a.nchunks)
			load_chunk(ch + gridDim.x); // in flight during the products
		if (MODE == 2)
			asm volatile("" : "+v"(cg));
		// ---- update: D = X + P (-Y), tiles (rt, cp + 2 u); V = P M
		{
			f32x16 acc[NT], vacc;
#pragma unroll
			for (int u = 0; u < NT; ++u) {
				const int c0l = XC0 + 32 * cp + lam;
#pragma unroll
				for (int g = 0; g < 4; ++g) {
					const f32x4 x = *reinterpret_cast<const f32x4 *>(&sm[c0l * TQ_LP + 32 * rt + 8 * g + 4 * h]);
#pragma unroll
					for (int e = 0; e < 4; ++e)
						acc[u][4 * g + e] = x[e];
				}
			}
#pragma unroll
			for (int r = 0; r < 16; ++r)
				vacc[r] = 0.f;
#pragma unroll
			for (int s2 = 0; s2 < 32; ++s2) {
				const float pv = sm[(2 * s2 + h) * TQ_LP + 32 * rt + lam];
#pragma unroll
				for (int u = 0; u < NT; ++u)
					if (act[u]) // (uniform)
						acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(pv, yreg[u][s2], acc[u], 0, 0, 0);
				if (MODE == 1 && vact)
					vacc = __builtin_amdgcn_mfma_f32_32x32x2f32(pv, mreg[s2], vacc, 0, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < NT; ++u)
				if (act[u]) {
					const int c0l = XC0 + 32 * cp + lam;
#pragma unroll
					for (int g = 0; g < 4; ++g)
						*reinterpret_cast<f32x4 *>(&sm[c0l * TQ_LP + 32 * rt + 8 * g + 4 * h]) =
							f32x4{acc[u][4 * g], acc[u][4 * g + 1], acc[u][4 * g + 2], acc[u][4 * g + 3]};
				}
			if (MODE == 1 && vact) {
#pragma unroll
				for (int g = 0; g < 4; ++g)
					*reinterpret_cast<f32x4 *>(&vs[(32 * cp + lam) * TQ_LP + 32 * rt + 8 * g + 4 * h]) =
						f32x4{vacc[4 * g], vacc[4 * g + 1], vacc[4 * g + 2], vacc[4 * g + 3]};
			}
		}
		tq_lds_barrier();
		// ---- store: the quads this thread staged
		{
			const int rbase = ch * 64 + quad * 4;
#pragma unroll
			for (int i = 0; i < NQ; ++i) {
				const int c = i * CGN + cg;
				if (c < TQ_PW) {
					if (MODE == 1 && a.do_v && c < a.w) {
						store_quad(a.P + (long) c * a.ld, rbase, *reinterpret_cast<const f32x4 *>(&vs[c * TQ_LP + quad * 4]));
						if (a.Pc)
							store_quad(a.Pc + (long) c * a.ldpc, rbase, *reinterpret_cast<const f32x4 *>(&sm[c * TQ_LP + quad * 4]));
					}
				} else if (c < 2 * TQ_PW) {
					if (MODE == 1 && c - TQ_PW < a.wn) {
						const f32x4 v = *reinterpret_cast<const f32x4 *>(&sm[c * TQ_LP + quad * 4]);
						store_quad(a.N + (long) (c - TQ_PW) * a.ld, rbase, v);
						if (ch == 0 && a.want_g)
							*reinterpret_cast<f32x4 *>(a.A1s + (c - TQ_PW) * 64 + quad * 4) = v;
					}
				} else if (c - 2 * TQ_PW < a.ts) {
					store_quad(a.F + (long) (c - 2 * TQ_PW) * a.ld, rbase, *reinterpret_cast<const f32x4 *>(&sm[c * TQ_LP + quad * 4]));
				}
			}
		}
		// ---- gram on the updated chunk (tq_gram_kernel's products with N in the place of its panel and F in the place of its X)
		if (MODE == 1 && a.want_g) {
			const int t0 = wv == 0 ? 0x30 : (wv == 1 ? 0x33 : (wv == 2 ? 0x22 : 0x00)); // (ia << 4) | ib
			const int t1 = wv == 0 ? 0x31 : (wv == 1 ? 0x20 : (wv == 2 ? 0x10 : -1));
			const int t2 = wv == 0 ? 0x32 : (wv == 1 ? 0x21 : (wv == 2 ? 0x11 : -1));
#pragma unroll
			for (int s4 = 0; s4 < 4; ++s4) {
				const int roff = 16 * s4 + 4 * (lane >> 4);
#pragma unroll
				for (int u = 0; u < 3; ++u) {
					const int tt = u == 0 ? t0 : (u == 1 ? t1 : t2);
					if (tt >= 0) { // wave uniform
						const f32x4 av = *reinterpret_cast<const f32x4 *>(&sm[(TQ_PW + 16 * (tt >> 4) + (lane & 15)) * TQ_LP + roff]);
						const f32x4 bv = *reinterpret_cast<const f32x4 *>(&sm[(TQ_PW + 16 * (tt & 15) + (lane & 15)) * TQ_LP + roff]);
#pragma unroll
						for (int q = 0; q < 4; ++q)
							gacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) av[q], (double) bv[q], gacc[u], 0, 0, 0);
					}
				}
			}
		}
		if (MODE == 2 && wv < ntile) { // tile wv of C': N half wv & 1, strip wv >> 1 of F
			const int ia = wv & 1, ib = wv >> 1;
#pragma unroll
			for (int s8 = 0; s8 < 8; ++s8) {
				const int roff = 8 * s8 + 4 * (lane >> 5);
				const f32x4 av = *reinterpret_cast<const f32x4 *>(&sm[(TQ_PW + 32 * ia + lam) * TQ_LP + roff]);
				const f32x4 bv = *reinterpret_cast<const f32x4 *>(&sm[(2 * TQ_PW + 32 * ib + lam) * TQ_LP + roff]);
#pragma unroll
				for (int q = 0; q < 4; ++q)
					cacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], cacc[0], 0, 0, 0);
			}
		}
	}
	const long blk = blockIdx.x;
	if (MODE == 1 && a.want_g) {
		const int t0 = wv == 0 ? 0x30 : (wv == 1 ? 0x33 : (wv == 2 ? 0x22 : 0x00));
		const int t1 = wv == 0 ? 0x31 : (wv == 1 ? 0x20 : (wv == 2 ? 0x10 : -1));
		const int t2 = wv == 0 ? 0x32 : (wv == 1 ? 0x21 : (wv == 2 ? 0x11 : -1));
#pragma unroll
		for (int u = 0; u < 3; ++u) {
			const int tt = u == 0 ? t0 : (u == 1 ? t1 : t2);
			if (tt >= 0) {
#pragma unroll
				for (int r = 0; r < 4; ++r)
					a.Gp[blk * 4096 + (16 * (tt >> 4) + (lane >> 4) + 4 * r) * 64 + 16 * (tt & 15) + (lane & 15)] = gacc[u][r];
			}
		}
	}
	if (MODE == 2 && wv < ntile) {
		const int ia = wv & 1, ib = wv >> 1;
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
			a.Cp[blk * 64 * a.tp + (long) (32 * ia + i) * a.tp + 32 * ib + lam] = cacc[0][r];
		}
	}
}

// ------------------------------------------------------------------------------------------------
// cross-panel blocks of T inside one block of Q_coeff, from small matrices only (no pass over V).
// After the block reflector of panel k has been applied,  V_k^T X' = -T_k Z_k  (T_k + T_k^T = V_k^T V_k), and every
// later reflector changes it by  -(V_k^T V_j) Z_j = -T_kj Z_j.  With V_l = (A~_l - [R_l; 0]) M_l below row c_l and zero above:
//   T_kl = V_k^T V_l = ( B_l - V_k[c_k : c_l + w_l, :]^T R[c_k : c_l + w_l, cols of l] ) M_l,
//   B = V_k^T X over all rows >= c_k:  B := -T_k Z_k after step k,  B[:, cols > l] -= T_kl Z_l[:, cols > l] after step l.
// (checked against the Gram matrix of the stored V in tests/diag/proto_tsqr.py: 0.1 eps.)  One workgroup per panel k, the
// blocks l = k + 1, ... of its block of Q_coeff in sequence; 64 x 64 x 64 products on the fp64 matrix cores.
// The first version computed these blocks as Gram products over V: three more passes, 0.46 of 3.4 ms.
// ------------------------------------------------------------------------------------------------
template <typename T> struct TqTxArgs {
	const T *A;
	long ld;
	int n, bs;
	const double *Td, *Md; // per panel 64 x 64
	const double *Z;       // per panel 64 x ldz
	int ldz;
	double *B; // scratch per panel 64 x ldz (general kernel); per panel 2 x 64 x 64: B_L and V^T R between the stages
	T *H;
	long hrs, hcs;
	const int *stat;
	int stage; // 0: everything; 1: all that does not need the LAST panel's kernel (runs beside it); 2: the rest
};

// acc[jb] (rows 16 wv .. + 15, columns 16 jb .. + 15) += A (64 x 64, LDS) * B (64 x 64, LDS)
static __device__ __forceinline__ void tq_mm64(f64x4 (&acc)[4], const double *Am, const double *Bm, int wv, int lane)
{
#pragma unroll 4
	for (int k0 = 0; k0 < 64; k0 += 4) {
		const double av = Am[(16 * wv + (lane & 15)) * TQ_DP + k0 + (lane >> 4)];
#pragma unroll
		for (int jb = 0; jb < 4; ++jb) {
			const double bv = Bm[(k0 + (lane >> 4)) * TQ_DP + 16 * jb + (lane & 15)];
			acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[jb], 0, 0, 0);
		}
	}
}

// The sequence of 64 x 64 x 64 products of one workgroup (panel k), in order; operands that come from global memory are
// fetched into registers one product ahead (the first version staged them behind two barriers per product and kept B in
// global memory: ~13 us per product, 238 us per factorization, all of it dependent memory round trips).
struct TqTxUnit {
	int type; // 0: B_l = -T_k Z_k[:, l];  1: acc += V_k^T chunk * R chunk;  2: T_kl = (B_l - acc) M_l;  3: B_l2 -= T_kl Z_l[:, l2];  4: done
	int l, x; // x: first row of the chunk (type 1) / l2 (type 3)
};

constexpr int TQ_TX_MAXL = 3; // later panels of one block of Q_coeff kept in registers (blocks of Q_coeff up to 256 columns)

template <typename T> __global__ __launch_bounds__(256) void tq_tx_kernel(const TqTxArgs<T> a)
{
	__shared__ double Am[64 * TQ_DP], Bm[64 * TQ_DP], Tm[64 * TQ_DP];
	if (a.stat[0])
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int k = blockIdx.x;
	const int ck = k * TQ_PW;
	const int bend = min(a.n, (ck / a.bs + 1) * a.bs); // end of the block of Q_coeff that holds panel k
	const int l1 = k + 1, lend = (bend + TQ_PW - 1) / TQ_PW; // panels l1 .. lend - 1 share the block
	if (l1 >= lend)
		return;
	auto next = [&](TqTxUnit u) {
		const int cl = u.l * TQ_PW, wl = min(TQ_PW, a.n - cl);
		if (u.type == 0) {
			if (u.l + 1 < lend)
				return TqTxUnit{0, u.l + 1, 0};
			return TqTxUnit{1, l1, ck};
		}
		if (u.type == 1) {
			if (u.x + 64 < cl + wl)
				return TqTxUnit{1, u.l, u.x + 64};
			return TqTxUnit{2, u.l, 0};
		}
		if (u.type == 2) {
			if (u.l + 1 < lend)
				return TqTxUnit{3, u.l, u.l + 1};
			return TqTxUnit{4, 0, 0};
		}
		if (u.x + 1 < lend)
			return TqTxUnit{3, u.l, u.x + 1};
		return TqTxUnit{1, u.l + 1, ck};
	};
	// element (i, j) = (e >> 6, e & 63), e = tid + 256 q, of the operands of a product.  Only what comes from global memory
	// is fetched ahead: the fp64 B operand of types 0 / 2 / 3 (rb) or the two fp32 chunks of type 1 (fa, fb); the A operand of
	// type 0 (T_k) is loaded once, those of types 2 / 3 are written to LDS by the previous epilogue
	auto fetch = [&](const TqTxUnit &u, double (&rb)[16], T (&fa)[16], T (&fb)[16]) {
		const int cl = u.l * TQ_PW, wl = min(TQ_PW, a.n - cl);
		if (u.type == 1) {
#pragma unroll
			for (int q = 0; q < 16; ++q) {
				// transposed fill: this thread handles row gr = x + (e & 63) of A and column ii = e >> 6 (lanes along the rows)
				const int e = tid + 256 * q, gr = u.x + (e & 63), ii = e >> 6;
				T va = 0, vb = 0;
				if (gr < cl + wl) {
					const int rr = gr - ck; // row inside V_k: unit lower trapezoid
					va = rr < ii ? (T) 0 : (rr == ii ? (T) 1 : a.A[(long) (ck + ii) * a.ld + gr]);
					if (ii < wl && !(gr - cl > ii)) // strictly below the diagonal of R_l the array holds V_l
						vb = a.A[(long) (cl + ii) * a.ld + gr];
				}
				fa[q] = va;
				fb[q] = vb;
			}
		} else {
			const double *pb;
			long ldb;
			int ncol = 64;
			if (u.type == 2) {
				pb = a.Md + (long) u.l * 4096;
				ldb = 64;
			} else {
				const int c0 = (u.type == 0 ? u.l : u.x) * TQ_PW;
				pb = a.Z + (long) (u.type == 0 ? k : u.l) * 64 * a.ldz + c0;
				ldb = a.ldz;
				ncol = a.n - c0;
			}
#pragma unroll
			for (int q = 0; q < 16; ++q) {
				const int e = tid + 256 * q, i = e >> 6, j = e & 63;
				rb[q] = j < ncol ? pb[(long) i * ldb + j] : 0.0;
			}
		}
	};
	auto stage = [&](const TqTxUnit &u, const double (&rb)[16], const T (&fa)[16], const T (&fb)[16]) {
#pragma unroll
		for (int q = 0; q < 16; ++q) {
			const int e = tid + 256 * q, i = e >> 6, j = e & 63;
			if (u.type == 1) { // Am[ii][row], Bm[row][ii]
				Am[i * TQ_DP + j] = (double) fa[q];
				Bm[j * TQ_DP + i] = (double) fb[q];
			} else {
				Bm[i * TQ_DP + j] = rb[q];
			}
		}
	};
	for (int e = tid; e < 4096; e += 256)
		Am[(e >> 6) * TQ_DP + (e & 63)] = a.Td[(long) k * 4096 + e]; // T_k: the A operand of the type-0 products
	f64x4 Bacc[TQ_TX_MAXL][4]; // B_l for the later panels: rows 16 wv .. + 15 (f64 16x16x4 result map: col = lane & 15, row = (lane >> 4) + 4 reg)
	f64x4 acc[4], vr[4];
#pragma unroll
	for (int li = 0; li < TQ_TX_MAXL; ++li)
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
			Bacc[li][jb] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int jb = 0; jb < 4; ++jb)
		vr[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
	double rb[16];
	T fa[16], fb[16];
	// Two stages: everything up to the last 64-row chunk of V_k^T R for the LAST panel L of the block needs nothing of panel
	// L's kernel (its R block and M) and runs on a second stream beside it; B_L and the partial V^T R travel through a.B.
	const int L = lend - 1, cL = L * TQ_PW;
	auto is_cut = [&](const TqTxUnit &t) { return t.type == 1 && t.l == L && t.x == cL; };
	double *state = a.B + (long) k * 2 * 4096;
	TqTxUnit u{0, l1, 0};
	if (a.stage == 2) {
		u = TqTxUnit{1, L, cL};
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int o = (16 * wv + (lane >> 4) + 4 * r) * 64 + 16 * jb + (lane & 15);
				vr[jb][r] = state[4096 + o];
#pragma unroll
				for (int q = 0; q < TQ_TX_MAXL; ++q)
					if (q == L - l1)
						Bacc[q][jb][r] = state[o];
			}
	}
	fetch(u, rb, fa, fb);
	while (u.type != 4) {
		if (a.stage == 1 && is_cut(u)) {
#pragma unroll
			for (int jb = 0; jb < 4; ++jb)
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const int o = (16 * wv + (lane >> 4) + 4 * r) * 64 + 16 * jb + (lane & 15);
					state[4096 + o] = vr[jb][r];
#pragma unroll
					for (int q = 0; q < TQ_TX_MAXL; ++q)
						if (q == L - l1)
							state[o] = Bacc[q][jb][r];
				}
			return; // (uniform)
		}
		__syncthreads(); // the previous product has read its operands
		stage(u, rb, fa, fb);
		__syncthreads();
		const TqTxUnit un = next(u);
		if (un.type != 4 && !(a.stage == 1 && is_cut(un)))
			fetch(un, rb, fa, fb); // in flight during the product
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
			acc[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
		tq_mm64(acc, u.type == 3 ? Tm : Am, Bm, wv, lane);
		const int li = u.l - l1;
		if (u.type == 0) {
#pragma unroll
			for (int q = 0; q < TQ_TX_MAXL; ++q)
				if (q == li)
#pragma unroll
					for (int jb = 0; jb < 4; ++jb)
						Bacc[q][jb] = -acc[jb];
		} else if (u.type == 1) {
#pragma unroll
			for (int jb = 0; jb < 4; ++jb)
				vr[jb] += acc[jb];
			if (un.type == 2) {
				// Am = B_l - V_k^T R (this wavefront's 16 rows: read by tq_mm64 of the next product after its barrier)
				__syncthreads(); // every wavefront has finished reading Am
#pragma unroll
				for (int q = 0; q < TQ_TX_MAXL; ++q)
					if (q == li)
#pragma unroll
						for (int jb = 0; jb < 4; ++jb)
#pragma unroll
							for (int r = 0; r < 4; ++r)
								Am[(16 * wv + (lane >> 4) + 4 * r) * TQ_DP + 16 * jb + (lane & 15)] = Bacc[q][jb][r] - vr[jb][r];
#pragma unroll
				for (int jb = 0; jb < 4; ++jb)
					vr[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
			}
		} else if (u.type == 2) {
			const int cl = u.l * TQ_PW, wl = min(TQ_PW, a.n - cl);
#pragma unroll
			for (int jb = 0; jb < 4; ++jb)
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const int i = 16 * wv + (lane >> 4) + 4 * r, j = 16 * jb + (lane & 15);
					Tm[i * TQ_DP + j] = acc[jb][r]; // read as the A operand of the type-3 products (behind their barriers)
					if (j < wl) {
						const int gi = ck + i, gj = cl + j;
						a.H[(long) (gi % a.bs) * a.hrs + (long) gj * a.hcs] = (T) acc[jb][r];
					}
				}
		} else {
			const int l2i = u.x - l1;
#pragma unroll
			for (int q = 0; q < TQ_TX_MAXL; ++q)
				if (q == l2i)
#pragma unroll
					for (int jb = 0; jb < 4; ++jb)
						Bacc[q][jb] -= acc[jb];
		}
		u = un;
	}
}

// General form (any number of later panels in the block of Q_coeff): B in global memory, operands staged per product.
template <typename T> __global__ __launch_bounds__(256) void tq_tx_general_kernel(const TqTxArgs<T> a)
{
	__shared__ double Am[64 * TQ_DP], Bm[64 * TQ_DP], Tm[64 * TQ_DP];
	if (a.stat[0])
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int k = blockIdx.x;
	const int ck = k * TQ_PW;
	const int bend = min(a.n, (ck / a.bs + 1) * a.bs); // end of the block of Q_coeff that holds panel k
	const int l1 = k + 1, lend = (bend + TQ_PW - 1) / TQ_PW; // panels l1 .. lend - 1 share the block
	if (l1 >= lend)
		return;
	double *Bk = a.B + (long) k * 64 * a.ldz;
	auto zero_acc = [](f64x4 (&acc)[4]) {
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
			acc[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
	};
	// f64 16x16x4 result map: col = lane & 15, row = (lane >> 4) + 4 * reg
	// ---- B := -T_k Z_k on the columns of the later panels of the block
	for (int e = tid; e < 4096; e += 256)
		Am[(e >> 6) * TQ_DP + (e & 63)] = a.Td[(long) k * 4096 + e];
	for (int l = l1; l < lend; ++l) {
		const int cl = l * TQ_PW;
		__syncthreads();
		for (int e = tid; e < 4096; e += 256) {
			const int i = e >> 6, j = e & 63;
			Bm[i * TQ_DP + j] = cl + j < a.n ? a.Z[((long) k * 64 + i) * a.ldz + cl + j] : 0.0;
		}
		__syncthreads();
		f64x4 acc[4];
		zero_acc(acc);
		tq_mm64(acc, Am, Bm, wv, lane);
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
#pragma unroll
			for (int r = 0; r < 4; ++r)
				Bk[(long) (16 * wv + (lane >> 4) + 4 * r) * a.ldz + cl + 16 * jb + (lane & 15)] = -acc[jb][r];
	}
	for (int l = l1; l < lend; ++l) {
		const int cl = l * TQ_PW;
		const int wl = min(TQ_PW, a.n - cl);
		// ---- acc = V_k[c_k : c_l + w_l, :]^T R[c_k : c_l + w_l, cols of l], 64 rows at a time
		f64x4 acc[4];
		zero_acc(acc);
		for (int r0 = ck; r0 < cl + wl; r0 += 64) {
			__syncthreads();
			for (int e = tid; e < 4096; e += 256) {
				const int i = e & 63, r = e >> 6; // Am[i][r] = V_k[r0 + r][i]: lanes along the rows of A (unit stride)
				const int gr = r0 + (e & 63), ii = e >> 6;
				// (transposed fill: thread e handles row gr, column ii -- consecutive threads read consecutive rows)
				double vv = 0.0;
				if (gr < cl + wl) {
					const int rr = gr - ck; // row inside V_k
					vv = rr < ii ? 0.0 : (rr == ii ? 1.0 : (double) a.A[(long) (ck + ii) * a.ld + gr]);
				}
				Am[ii * TQ_DP + (gr - r0)] = vv;
				double rv = 0.0;
				if (gr < cl + wl && ii < wl) {
					const bool below = gr - cl > ii; // strictly below the diagonal of R_l: holds V_l, not R
					rv = below ? 0.0 : (double) a.A[(long) (cl + ii) * a.ld + gr];
				}
				Bm[(gr - r0) * TQ_DP + ii] = rv;
				(void) i;
				(void) r;
			}
			__syncthreads();
			tq_mm64(acc, Am, Bm, wv, lane);
		}
		// ---- Tm = B_l - acc, then T_kl = Tm M_l
		__syncthreads();
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int i = 16 * wv + (lane >> 4) + 4 * r, j = 16 * jb + (lane & 15);
				Am[i * TQ_DP + j] = Bk[(long) i * a.ldz + cl + j] - acc[jb][r];
			}
		for (int e = tid; e < 4096; e += 256)
			Bm[(e >> 6) * TQ_DP + (e & 63)] = a.Md[(long) l * 4096 + e];
		__syncthreads();
		zero_acc(acc);
		tq_mm64(acc, Am, Bm, wv, lane);
#pragma unroll
		for (int jb = 0; jb < 4; ++jb)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int i = 16 * wv + (lane >> 4) + 4 * r, j = 16 * jb + (lane & 15);
				Tm[i * TQ_DP + j] = acc[jb][r];
				if (j < wl) {
					const int gi = ck + i, gj = cl + j;
					a.H[(long) (gi % a.bs) * a.hrs + (long) gj * a.hcs] = (T) acc[jb][r];
				}
			}
		// ---- B[:, later panels] -= T_kl Z_l[:, later panels]
		for (int l2 = l + 1; l2 < lend; ++l2) {
			const int c2 = l2 * TQ_PW;
			__syncthreads();
			for (int e = tid; e < 4096; e += 256) {
				const int i = e >> 6, j = e & 63;
				Bm[i * TQ_DP + j] = c2 + j < a.n ? a.Z[((long) l * 64 + i) * a.ldz + c2 + j] : 0.0;
			}
			__syncthreads();
			zero_acc(acc);
			tq_mm64(acc, Tm, Bm, wv, lane);
#pragma unroll
			for (int jb = 0; jb < 4; ++jb)
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const long o = (long) (16 * wv + (lane >> 4) + 4 * r) * a.ldz + c2 + 16 * jb + (lane & 15);
					Bk[o] -= acc[jb][r];
				}
		}
		__syncthreads(); // Bk written by this workgroup is read by it in the next round (workgroup-scope visibility)
	}
}

// ------------------------------------------------------------------------------------------------
// fp64 data (round 6): the same factorization with Gram products and updates on the fp64 matrix cores.  Two streaming kernels of
// their own -- an fp64 chunk is twice the bytes, v_mfma_f64_16x16x4 has another operand shape -- everything else (reduce, panel, y,
// T blocks) is the code above instantiated for double.  Schedule: the plain one (Gram, panel, y, update per panel on one stream).
// ------------------------------------------------------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int TQ_LP64 = 18; // LDS pitch (doubles) of one staged column of a 16-row chunk: 16-byte aligned (36 dwords: the 16 lanes of a b128 group hit distinct banks but for two pairs)

// 16-byte vectors of the scalar type: RPV consecutive rows of a column per load / store
template <typename T> struct TqVec;
template <> struct TqVec<double> {
	typedef f64x2 v;
	static constexpr int RPV = 2;
};

template <typename T> struct TqGramTArgs {
	const T *P; // A[r0, c0]
	const T *X; // A[r0, cx]
	long ld;
	int rows, w, t, tp; // rows from r0 down, panel width, trailing columns of this launch, t rounded up to 64 (32 NC)
	int nsub, nchunks;  // sub-chunks (8 RPV rows each) per chunk (4 / 2 / 1 for <= 64 / <= 128 / more staged columns), chunks
	int want_g, want_sq;
	double *Gp; // [grid][64 * 64]
	T *Cp;	    // [grid][64 * tp]
	T *Sp;	    // [grid][256]
	const int *stat;
	int c0;
	T *A1s; // want_g: the panel's top 64 x 64 block, column major
};

// bounds-checked 16-byte access (the partial chunk of a launch, views whose rows are not 16-byte aligned)
template <typename T, bool VEC> static __device__ __forceinline__ typename TqVec<T>::v tq_ldv(const T *p, int r, int rows)
{
	constexpr int RPV = TqVec<T>::RPV;
	typename TqVec<T>::v v;
#pragma unroll
	for (int e = 0; e < RPV; ++e)
		v[e] = (T) 0;
	if (VEC && r + RPV - 1 < rows) {
		v = *reinterpret_cast<const typename TqVec<T>::v *>(p + r);
	} else {
#pragma unroll
		for (int e = 0; e < RPV; ++e)
			if (r + e < rows)
				v[e] = p[r + e];
	}
	return v;
}
template <typename T, bool VEC> static __device__ __forceinline__ void tq_stv(T *p, int r, int rows, typename TqVec<T>::v v)
{
	constexpr int RPV = TqVec<T>::RPV;
	if (VEC && r + RPV - 1 < rows) {
		*reinterpret_cast<typename TqVec<T>::v *>(p + r) = v;
	} else {
#pragma unroll
		for (int e = 0; e < RPV; ++e)
			if (r + e < rows)
				p[r + e] = v[e];
	}
}

// G = P^T P (lower 16 x 16 tiles, fp64 matrix cores: for fp32 data the products are exact) and C = P^T X (matrix cores of the scalar
// type), per-workgroup partial sums.  One persistent workgroup of 512 threads per CU.  A chunk is 32 KB of [P | X]: one sub-chunk
// (8 RPV rows: 16 of fp64, 32 of fp32) of <= 256 columns, or -- narrow launches -- 2 / 4 sub-chunks of <= 128 / 64 columns side by
// side (a single sub-chunk of 64 columns is 8 KB: a memory round trip per 8 KB).  Thread (q = tid & 7, cg = tid >> 3) loads rows
// RPV q .. of the staged columns cg + 64 i: eight lanes cover the 128 bytes a column contributes to a sub-chunk.  FOUR chunks per
// workgroup are in flight in registers (64 staging registers) and the LDS image is double buffered: per chunk ONE barrier that
// leaves the global loads in flight; the first version (two 256-thread workgroups per CU, one chunk ahead each) ran at
// 2.1-2.4 TB/s.  Wavefront (ia = wv & 3, hf = wv >> 2) owns the panel columns 16 ia .. + 15 (rows of G and C) and every other
// column tile: its A operand is read once per sub-chunk, the B operand once per tile; lane (i = l & 15, g = l >> 4) takes the rows
// KS g .. KS g + KS - 1 of its column (KS = 2 RPV) as k-slices -- the order of the rows inside a Gram sum is free.
// Balance (fp64) at t = 192: 58 tiles x 4 MFMAs x 64 cycles per 32 KB chunk and four SIMDs = 4.5-4.8 TB/s chip-wide at the fp64
// matrix-core peak: the kernel is bound by both at once.
template <typename T, int NC, bool VEC> __global__ __launch_bounds__(512, 1) void tq_gramT_kernel(const TqGramTArgs<T> a)
{
	typedef typename TqVec<T>::v vec_t;
	typedef typename Mfma<T>::acc_t cacc_t;
	constexpr int RPV = TqVec<T>::RPV;
	constexpr int SR = 8 * RPV;   // rows of a sub-chunk
	constexpr int KS = 2 * RPV;   // k-slices of a lane per sub-chunk (32 bytes: two vectors)
	constexpr int LP = SR + RPV;  // LDS pitch of a staged column (18 doubles / 36 floats = 36 dwords: see TQ_LP64)
	static_assert(LP * sizeof(T) == TQ_LP64 * 8, "pitch");
	__shared__ T sm[2][256 * LP];
	if (tq_skip(a.stat, a.c0))
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int ia = wv & 3, hf = wv >> 2;
	const int q = tid & 7, cg = tid >> 3;
	const int ncol = TQ_PW + a.tp;
	const int nslot = (ncol + 63) >> 6;	      // 64-column load slots per sub-chunk: 1 .. 4
	const int nsub = a.nsub;		      // sub-chunks per chunk: 4 / nslot
	const int ncolp = nslot * 64;		      // staged columns per sub-chunk
	f64x4 gacc[2];
	cacc_t cacc[NC > 0 ? NC : 1];
#pragma unroll
	for (int i = 0; i < 2; ++i)
		gacc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int i = 0; i < (NC > 0 ? NC : 1); ++i)
#pragma unroll
		for (int r = 0; r < 4; ++r)
			cacc[i][r] = (T) 0;
	double sq[4] = {0.0, 0.0, 0.0, 0.0};
	// slot i of a thread: sub-chunk si, column ci of [P | X]; a slot without a column (a column beyond the launch's, the fourth slot of
	// a 192-column chunk) loads from column 0 of the panel and stages zeros into a part of the image no product reads
	int ldsoff[4], roff[4];
	bool act[4];
	const T *colp[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int si = i / nslot, ci = (i - si * nslot) * 64 + cg;
		const bool isp = ci < TQ_PW;
		const int cc = isp ? ci : ci - TQ_PW;
		act[i] = si < nsub && (isp ? cc < a.w : cc < a.t);
		colp[i] = act[i] ? (isp ? a.P : a.X) + (long) cc * a.ld : a.P;
		roff[i] = act[i] ? SR * si + RPV * q : RPV * q;
		ldsoff[i] = (si * ncolp + ci) * LP + RPV * q; // (si * ncolp + ci < 256 always)
	}
	// unconditional load of RPV consecutive rows: one 16-byte load, or -- columns that are not 16-byte aligned (a view that starts at an
	// odd row, an odd column stride) -- RPV scalar loads, still without a branch
	auto ldu = [](const T *p) {
		vec_t v;
		if (VEC) {
			v = *reinterpret_cast<const vec_t *>(p);
		} else {
#pragma unroll
			for (int x = 0; x < RPV; ++x)
				v[x] = p[x];
		}
		return v;
	};
	const int crows = SR * nsub;
	// A workgroup owns a contiguous run of FULL chunks; the partial chunk at the end of the matrix (if any) is the last workgroup's
	// epilogue.  The main loop is straight-line code: unconditional 16-byte loads, counted waits.  (Loads under per-lane branches --
	// the bounds checks of the first version -- share their destination registers with the scalar loads of the other branch, the
	// compiler drained the memory counter in front of every one of them and the kernel streamed at 2.3 TB/s whatever it did with
	// the data: one round trip per load.)
	const int nfull = a.rows / crows;
	const int cpw = (nfull + (int) gridDim.x - 1) / (int) gridDim.x;
	const int first = (int) blockIdx.x * cpw;
	const int nmine = nfull - first < 0 ? 0 : (nfull - first < cpw ? nfull - first : cpw);
	if (blockIdx.x == 0 && a.want_g) {
		// the panel's top block for the panel kernel (64 rows: rows >= 3 n)
		for (int e = tid; e < 64 * (64 / RPV); e += 512) {
			const int c = e / (64 / RPV), rp = e % (64 / RPV);
			vec_t v;
#pragma unroll
			for (int x = 0; x < RPV; ++x)
				v[x] = (T) 0;
			if (c < a.w)
				v = ldu(a.P + (long) c * a.ld + RPV * rp);
			*reinterpret_cast<vec_t *>(a.A1s + c * 64 + RPV * rp) = v;
		}
	}
	vec_t s0[4], s1[4], s2[4], s3[4];
	auto load_chunk = [&](int j, vec_t (&st)[4]) { // chunk min(j, nmine - 1) of this workgroup
		const int jj = j < nmine ? j : nmine - 1;
		const long r0 = (long) (first + jj) * crows;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			st[i] = ldu(colp[i] + r0 + roff[i]);
	};
	auto stage = [&](int j, const vec_t (&st)[4], double count) { // into LDS half j & 1
		T *dst = sm[j & 1];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			vec_t v = st[i];
			double s = 0.0;
#pragma unroll
			for (int x = 0; x < RPV; ++x) {
				v[x] = act[i] ? v[x] : (T) 0;
				s += (double) v[x] * (double) v[x];
			}
			*reinterpret_cast<vec_t *>(&dst[ldsoff[i]]) = v;
			sq[i] += count * s;
		}
	};
	// NC column tiles of C per wavefront (a.tp == 32 NC): the B operands of two tiles are requested together, consecutive MFMAs go to
	// different accumulators
	auto products = [&](int j) {
		const T *src = sm[j & 1];
		const int ro = KS * (lane >> 4);
#pragma unroll 1
		for (int sb = 0; sb < nsub; ++sb) {
			const T *base = src + (long) sb * ncolp * LP + (lane & 15) * LP + ro;
			const T *ap = base + 16 * ia * LP;
			const vec_t alo = *reinterpret_cast<const vec_t *>(ap), ahi = *reinterpret_cast<const vec_t *>(ap + RPV);
#pragma unroll
			for (int c0 = 0; c0 < NC; c0 += 2) {
				vec_t blo[2], bhi[2];
#pragma unroll
				for (int c = 0; c < 2; ++c) {
					const T *bp = base + (TQ_PW + 16 * (2 * (c0 + c) + hf)) * LP;
					blo[c] = *reinterpret_cast<const vec_t *>(bp);
					bhi[c] = *reinterpret_cast<const vec_t *>(bp + RPV);
				}
#pragma unroll
				for (int x = 0; x < RPV; ++x)
#pragma unroll
					for (int c = 0; c < 2; ++c)
						cacc[c0 + c] = Mfma<T>::run(alo[x], blo[c][x], cacc[c0 + c]);
#pragma unroll
				for (int x = 0; x < RPV; ++x)
#pragma unroll
					for (int c = 0; c < 2; ++c)
						cacc[c0 + c] = Mfma<T>::run(ahi[x], bhi[c][x], cacc[c0 + c]);
			}
			if (a.want_g) {
#pragma unroll
				for (int u = 0; u < 2; ++u) {
					const int jb = 2 * hf + u;
					if (jb <= ia) { // wave uniform
						const T *bp = base + 16 * jb * LP;
						const vec_t glo = *reinterpret_cast<const vec_t *>(bp), ghi = *reinterpret_cast<const vec_t *>(bp + RPV);
#pragma unroll
						for (int x = 0; x < RPV; ++x)
							gacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) alo[x], (double) glo[x], gacc[u], 0, 0, 0);
#pragma unroll
						for (int x = 0; x < RPV; ++x)
							gacc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double) ahi[x], (double) ghi[x], gacc[u], 0, 0, 0);
					}
				}
			}
		}
	};
	// chunk j lives in staging buffer j & 3; step j: chunk j + 1 into the other LDS half, its buffer refilled with chunk j + 5,
	// the products of chunk j, one barrier (that leaves the global loads in flight).  Beyond the workgroup's last chunk the steps
	// reload and restage that chunk (never consumed, not counted in the column squares): no branch around a load.
	if (nmine > 0) {
		load_chunk(0, s0);
		load_chunk(1, s1);
		load_chunk(2, s2);
		load_chunk(3, s3);
		stage(0, s0, 1.0);
		load_chunk(4, s0);
		tq_lds_barrier();
#define TQ_GT_STEP(J, SN)                                                                                                                   \
	{                                                                                                                                   \
		stage((J) + 1, SN, (J) + 1 < nmine ? 1.0 : 0.0);                                                                            \
		load_chunk((J) + 5, SN);                                                                                                    \
		products(J);                                                                                                                \
		tq_lds_barrier();                                                                                                           \
	}
		int j = 0;
#pragma unroll 1
		for (; j + 3 < nmine; j += 4) {
			TQ_GT_STEP(j, s1)
			TQ_GT_STEP(j + 1, s2)
			TQ_GT_STEP(j + 2, s3)
			TQ_GT_STEP(j + 3, s0)
		}
		// (the last 0 .. 3 chunks)
		if (j < nmine)
			TQ_GT_STEP(j, s1)
		if (j + 1 < nmine)
			TQ_GT_STEP(j + 1, s2)
		if (j + 2 < nmine)
			TQ_GT_STEP(j + 2, s3)
#undef TQ_GT_STEP
	}
	if (blockIdx.x == gridDim.x - 1 && nfull * crows < a.rows) {
		// the partial chunk: bounds-checked loads
		const long r0 = (long) nfull * crows;
#pragma unroll
		for (int i = 0; i < 4; ++i) {
#pragma unroll
			for (int x = 0; x < RPV; ++x)
				s0[i][x] = (T) 0;
			if (act[i])
				s0[i] = tq_ldv<T, VEC>(colp[i] + r0, roff[i], a.rows - (int) r0);
		}
		__syncthreads();
		stage(0, s0, 1.0);
		__syncthreads();
		products(0);
	}
	// result map of the 16x16x4 forms: col = lane & 15, row = Mfma<.>::row(reg, lane >> 4)
	const long blk = blockIdx.x;
	if (a.want_g) {
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int jb = 2 * hf + u;
			if (jb <= ia) {
#pragma unroll
				for (int r = 0; r < 4; ++r)
					a.Gp[blk * 4096 + (16 * ia + Mfma<double>::row(r, lane >> 4)) * 64 + 16 * jb + (lane & 15)] = gacc[u][r];
			}
		}
	}
#pragma unroll
	for (int c = 0; c < NC; ++c) {
		const int cb = 2 * c + hf;
#pragma unroll
		for (int r = 0; r < 4; ++r)
			a.Cp[blk * 64 * a.tp + (long) (16 * ia + Mfma<T>::row(r, lane >> 4)) * a.tp + 16 * cb + (lane & 15)] = cacc[c][r];
	}
	if (a.want_sq) {
		// the slots of a thread that hold the same column (sub-chunks) are added in a fixed order
		if (nslot == 1) {
			sq[0] = (sq[0] + sq[1]) + (sq[2] + sq[3]);
		} else if (nslot == 2) {
			sq[0] += sq[2];
			sq[1] += sq[3];
		}
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			double v = sq[i];
			v += __shfl_xor(v, 1);
			v += __shfl_xor(v, 2);
			v += __shfl_xor(v, 4);
			if (q == 0 && i < nslot)
				a.Sp[blk * 256 + i * 64 + cg] = (T) v;
		}
	}
}

// update: X <- X - P Y on a strip of <= 192 trailing columns and, if do_v, V = P M over the panel (at most 16 column tiles of 16
// together: the whole trailing matrix of a 256-column factorization in ONE launch per panel).  The result tile is the TRANSPOSE of
// the strip's tile: D[i][j] = X[row j][column i] (lanes along the rows), so the A operand is (-Y)^T / M^T -- kept in registers for
// the whole launch, tiles wv and wv + 8 belong to wavefront wv of eight -- and the B operand the panel rows, staged per chunk of
// 16 RPV rows (32 of fp64, 64 of fp32) through LDS (16 KB).  A lane owns RPV consecutive rows of a chunk: 16-byte loads and stores,
// RPV tiles per column tile.  The strip's tiles and the panel rows of the NEXT chunk are loaded before the products of this one
// (first version: the strip's loads at the head of their own iteration, two 256-thread workgroups per CU covering for each other:
// 3.2-3.4 TB/s).  Chunks are visited from the last rows up: the Gram pass in front of this launch ended there, the one behind it
// starts at the top.  Balance (fp64): 2 x 64 x 16 x 32 flop per 8 KB read + written: at the fp64 matrix-core peak the strip would
// stream at 9-11 TB/s -- the kernel is HBM bound.
template <typename T> struct TqUpdTArgs {
	T *P; // A[r1, c0], r1 = first row below the top block
	T *X; // A[r1, cx + coff]
	long ld;
	int rows, w, ts; // rows from r1 down; strip width
	const T *Yn;	 // -Y, row major 64 x typ
	int typ, coff;
	const T *Mn; // M, row major 64 x 64
	int do_v;
	int nchunks; // chunks of 16 RPV rows
	const int *stat;
	int c0;
};

template <typename T, bool VEC> __global__ __launch_bounds__(512, 1) void tq_updateT_kernel(const TqUpdTArgs<T> a)
{
	typedef typename TqVec<T>::v vec_t;
	typedef typename Mfma<T>::acc_t acc_t;
	constexpr int RPV = TqVec<T>::RPV;
	constexpr int CR = 16 * RPV;  // rows of a chunk
	constexpr int LPP = CR + RPV; // LDS pitch of a staged panel column
	__shared__ T Pl[64 * LPP];
	if (tq_skip(a.stat, a.c0))
		return;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int li = lane & 15, g = lane >> 4;
	const int nx = (a.ts + 15) >> 4;
	const int nt = nx + (a.do_v ? 4 : 0);
	// A operands: ya[u][ks] = A[i = li][k = 4 ks + g] of tile wv + 8 u
	T ya[2][16];
#pragma unroll
	for (int u = 0; u < 2; ++u) {
		const int tl = wv + 8 * u;
		const bool isx = tl < nx, isv = !isx && tl < nt;
		const int col = isx ? 16 * tl + li : 16 * (tl - nx) + li;
		const bool ok = isx ? col < a.ts : (isv && col < a.w);
		const T *src = isx ? a.Yn + a.coff + col : a.Mn + col;
		const long step = isx ? (long) a.typ : 64L;
#pragma unroll
		for (int ks = 0; ks < 16; ++ks)
			ya[u][ks] = ok && (4 * ks + g) < a.w ? src[(long) (4 * ks + g) * step] : (T) 0;
	}
	const int pq = tid & 15, pc = tid >> 4; // staging: rows RPV pq .. of the panel columns pc, pc + 32
	vec_t pst[2];
	vec_t xv[2][4], xn[2][4];
	// chunk ch of the launch is rows CR (nchunks - 1 - ch) ..: chunk 0 is the one that may be partial.  Register r of a result tile is
	// the strip's column Mfma<T>::row(r, g) of the tile.
	auto load_checked = [&](int ch, vec_t (&x)[2][4]) {
		const int cr = a.nchunks - 1 - ch;
		const int rb = cr * CR + RPV * pq, rbase = cr * CR + RPV * li;
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			const int c = pc + 32 * i;
#pragma unroll
			for (int e = 0; e < RPV; ++e)
				pst[i][e] = (T) 0;
			if (c < a.w)
				pst[i] = tq_ldv<T, VEC>(a.P + (long) c * a.ld, rb, a.rows);
		}
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int tl = wv + 8 * u;
#pragma unroll
			for (int r = 0; r < 4; ++r) {
#pragma unroll
				for (int e = 0; e < RPV; ++e)
					x[u][r][e] = (T) 0;
				const int col = 16 * tl + Mfma<T>::row(r, g);
				if (tl < nx && col < a.ts)
					x[u][r] = tq_ldv<T, VEC>(a.X + (long) col * a.ld, rbase, a.rows);
			}
		}
	};
	// a chunk inside the matrix: unconditional 16-byte loads (see tq_gramT_kernel) -- panel columns beyond w read column 0 and are
	// zeroed when staged, tiles beyond the strip read a valid column and never use or store it
	const T *pcol[2], *xcol[2][4];
#pragma unroll
	for (int i = 0; i < 2; ++i)
		pcol[i] = a.P + (long) (pc + 32 * i < a.w ? pc + 32 * i : 0) * a.ld + RPV * pq;
#pragma unroll
	for (int u = 0; u < 2; ++u)
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int col = 16 * (wv + 8 * u) + Mfma<T>::row(r, g);
			xcol[u][r] = (a.ts > 0 ? a.X + (long) (col < a.ts ? col : a.ts - 1) * a.ld : a.P) + RPV * li;
		}
	auto load_full = [&](int ch, vec_t (&x)[2][4]) {
		const long r0 = (long) (a.nchunks - 1 - ch) * CR;
#pragma unroll
		for (int i = 0; i < 2; ++i)
			pst[i] = *reinterpret_cast<const vec_t *>(pcol[i] + r0);
#pragma unroll
		for (int u = 0; u < 2; ++u)
#pragma unroll
			for (int r = 0; r < 4; ++r)
				x[u][r] = *reinterpret_cast<const vec_t *>(xcol[u][r] + r0);
	};
	auto stage_panel = [&]() {
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			vec_t v = pst[i];
#pragma unroll
			for (int e = 0; e < RPV; ++e)
				v[e] = pc + 32 * i < a.w ? v[e] : (T) 0;
			*reinterpret_cast<vec_t *>(&Pl[(pc + 32 * i) * LPP + RPV * pq]) = v;
		}
	};
	auto compute_store = [&](int ch, const vec_t (&x)[2][4]) {
		const int rbase = (a.nchunks - 1 - ch) * CR + RPV * li;
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int tl = wv + 8 * u;
			if (tl < nt) { // wave uniform
				const bool isx = tl < nx;
				acc_t acc[RPV];
#pragma unroll
				for (int e = 0; e < RPV; ++e)
#pragma unroll
					for (int r = 0; r < 4; ++r)
						acc[e][r] = isx ? x[u][r][e] : (T) 0;
#pragma unroll
				for (int ks = 0; ks < 16; ++ks) {
					const vec_t b = *reinterpret_cast<const vec_t *>(&Pl[(4 * ks + g) * LPP + RPV * li]);
#pragma unroll
					for (int e = 0; e < RPV; ++e)
						acc[e] = Mfma<T>::run(ya[u][ks], b[e], acc[e]);
				}
				T *dst = isx ? a.X + (long) (16 * tl) * a.ld : a.P + (long) (16 * (tl - nx)) * a.ld;
				const int nvalid = isx ? a.ts - 16 * tl : a.w - 16 * (tl - nx);
#pragma unroll
				for (int r = 0; r < 4; ++r) {
					const int cl = Mfma<T>::row(r, g);
					vec_t o;
#pragma unroll
					for (int e = 0; e < RPV; ++e)
						o[e] = acc[e][r];
					if (cl < nvalid)
						tq_stv<T, VEC>(dst + (long) cl * a.ld, rbase, a.rows, o);
				}
			}
		}
	};
	// a workgroup owns a contiguous run of chunks
	const int cpw = (a.nchunks + (int) gridDim.x - 1) / (int) gridDim.x;
	int ch = (int) blockIdx.x * cpw;
	const int chend = ch + cpw < a.nchunks ? ch + cpw : a.nchunks;
	const int nchecked = VEC ? ((a.rows % CR) != 0 ? 1 : 0) : a.nchunks; // chunks [0, nchecked) take the bounds-checked path
	for (; ch < chend && ch < nchecked; ++ch) {
		load_checked(ch, xv);
		__syncthreads();
		stage_panel();
		__syncthreads();
		compute_store(ch, xv);
	}
	if (ch >= chend)
		return;
	// main loop, straight-line: the strip's tiles and the panel rows of the NEXT chunk are requested before the products of this one
	// (beyond the run's last chunk: that chunk again, never used)
	load_full(ch, xv);
#pragma unroll 1
	for (; ch < chend; ++ch) {
		tq_lds_barrier(); // the previous chunk's panel rows have been consumed (a barrier that leaves the global loads in flight)
		stage_panel();
		tq_lds_barrier();
		load_full(ch + 1 < chend ? ch + 1 : ch, xn);
		compute_store(ch, xv);
#pragma unroll
		for (int u = 0; u < 2; ++u)
#pragma unroll
			for (int r = 0; r < 4; ++r)
				xv[u][r] = xn[u][r];
	}
}

// ------------------------------------------------------------------------------------------------
// driver
// ------------------------------------------------------------------------------------------------
// V = P M over a panel: one persistent workgroup per CU of the `ncu` it may use (its registers and LDS allow no second one)
static void tq_launch_form_v(bool vec, int ncu, const TqFormVArgs &va)
{
	hipStream_t s = ctx().stream;
	const int nwg = (va.nrb + 3) / 4 < ncu ? (va.nrb + 3) / 4 : ncu;
	// (profile class 2; algorithmic bytes of the launch: the panel read once, V written once)
	ProfScope prof(2, (double) va.rows * 4.0 * 2.0 * (double) va.w);
	if (vec)
		hipLaunchKernelGGL(tq_form_v_kernel<true>, dim3(nwg), dim3(256), 0, s, va);
	else
		hipLaunchKernelGGL(tq_form_v_kernel<false>, dim3(nwg), dim3(256), 0, s, va);
}

static void tq_gram(const float *P, const float *X, long ld, int rows, int w, int t, bool want_g, bool want_sq, bool vec, double *Gp, float *Cp,
		    float *Sp, double *G, double *C, int ldc, int coff, double *S, const int *stat, int c0, float *A1s, double *Gf, int *cnt, int nb_max)
{
	hipStream_t s = ctx().stream;
	TqGramArgs g;
	g.A1s = A1s;
	g.P = P;
	g.X = X;
	g.ld = ld;
	g.rows = rows;
	g.w = w;
	g.t = t;
	g.tp = (t + 31) & ~31;
	g.nchunks = (rows + 63) / 64;
	g.want_g = want_g;
	g.want_sq = want_sq;
	g.Gp = Gp;
	g.Cp = Cp;
	g.Sp = Sp;
	g.stat = stat;
	g.c0 = c0;
	const int nbmax = nb_max > 0 && nb_max < TQ_NB ? nb_max : TQ_NB;
	const int nb = g.nchunks < nbmax ? g.nchunks : nbmax;
	if (nb <= 0)
		return;
	{
		ProfScope prof(3, (double) rows * 4.0 * ((double) w + (double) t)); // (class 3: the panel and the trailing columns read once)
		if (vec)
			hipLaunchKernelGGL(tq_gram_kernel<true>, dim3(nb), dim3(256), 0, s, g);
		else
			hipLaunchKernelGGL(tq_gram_kernel<false>, dim3(nb), dim3(256), 0, s, g);
	}
	const int total = (want_g ? 4096 : 0) + 64 * g.tp + (want_sq ? 256 : 0);
	hipLaunchKernelGGL(tq_reduce_kernel<float>, dim3((total + 255) / 256, TQ_NG), dim3(256), 0, s, Gp, Cp, Sp, nb, g.tp, (int) want_g, (int) want_sq, G, C,
			   ldc, coff, S, stat, c0, Gf, cnt);
	FH_HIP(hipGetLastError());
}

static std::atomic<int> g_tq_panel_copy{1};
void tsqr_debug_panel_copy(int on) { g_tq_panel_copy.store(on); }

static void tq_launch_fused(bool vec, int mode, int nwg, const TqFusedArgs &fa)
{
	hipStream_t s = ctx().stream;
	// (profile class 2; algorithmic bytes of the launch: everything staged read once, N / F / V written once)
	ProfScope prof(2, (double) fa.rows * 4.0 *
				  ((double) fa.w + (double) fa.wn + (mode == 1 ? (double) fa.wn + (fa.do_v ? (double) fa.w : 0.0) : 2.0 * (double) fa.ts)));
	if (mode == 1) {
		if (vec)
			hipLaunchKernelGGL((tq_fused_kernel<true, 1>), dim3(nwg), dim3(256), 0, s, fa);
		else
			hipLaunchKernelGGL((tq_fused_kernel<false, 1>), dim3(nwg), dim3(256), 0, s, fa);
	} else {
		if (vec)
			hipLaunchKernelGGL((tq_fused_kernel<true, 2>), dim3(nwg), dim3(512), 0, s, fa);
		else
			hipLaunchKernelGGL((tq_fused_kernel<false, 2>), dim3(nwg), dim3(512), 0, s, fa);
	}
}

// side streams of the factorization (owned by the per-thread context, ctx.hip): the panel kernel of step k + 1 (one
// workgroup) beside the rest of step k's update, and the cross-panel T blocks beside the last steps
struct TqSide {
	hipStream_t panel, tx;
	hipEvent_t pfork, pdone, xfork, xdone;
};
static TqSide tq_side()
{
	Ctx &c = ctx();
	c.qr_side_streams();
	return TqSide{c.qr_side[0], c.qr_side[1], c.qr_ev[0], c.qr_ev[1], c.qr_ev[2], c.qr_ev[3]};
}

// A matrix that is a sub-block of a larger one whose rows above it belong to the same columns (a panel of the classic path, qr.hip):
// the reference's rank test takes the norm of ALL rows above the diagonal (factor.rs:26,52-58), so abv starts from the squares of the
// `top` entries above each column.  One workgroup per column, fixed summation order.
template <typename T> __global__ __launch_bounds__(256) void tq_above_kernel(const T *A, long ld, int top, double *abv)
{
	__shared__ double red[256];
	const T *col = A + (long) blockIdx.x * ld;
	double sq = 0.0;
	for (int i = 1 + (int) threadIdx.x; i <= top; i += 256) {
		const double v = (double) col[-(long) i];
		sq += v * v;
	}
	red[threadIdx.x] = sq;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if ((int) threadIdx.x < o)
			red[threadIdx.x] += red[threadIdx.x + o];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		abv[blockIdx.x] = red[0];
}

// Range guard of the columns the first step's Gram launches do not cover (n > 256: the squares of the first 64 + 192
// columns come out of those launches, tq_panel_kernel / tq_y_kernel check them): one workgroup per column, BEFORE anything is
// written -- a column whose rms is outside [1e-12, 1e12] would be updated by the first steps with flushed or overflowed fp32
// products, and a later rejection could not undo that.  One more read of those columns (n <= 512).
template <typename T> __global__ __launch_bounds__(256) void tq_range_rest_kernel(const T *A, long ld, int m, int c_first, int *stat)
{
	__shared__ double red[256];
	const T *col = A + (long) (c_first + (int) blockIdx.x) * ld;
	double sq = 0.0;
	for (int i = threadIdx.x; i < m; i += 256) {
		const double v = (double) col[i];
		sq += v * v;
	}
	red[threadIdx.x] = sq;
	__syncthreads();
	for (int o = 128; o > 0; o >>= 1) {
		if ((int) threadIdx.x < o)
			red[threadIdx.x] += red[threadIdx.x + o];
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const double lo = TqLim<T>::sq_lo * (double) m, hi = TqLim<T>::sq_hi * (double) m;
		if (!(red[0] >= lo && red[0] <= hi)) {
			stat[1] = 0;
			stat[2] = TQ_FAIL_RANGE;
			__threadfence();
			atomicExch(stat, 1); // "stopped in front of column 0": every later kernel returns at once
		}
	}
}

// shape rule of the whole-matrix one-pass path: at least g_tq_min_rows rows and g_tq_min_aspect rows per column
// (rounds 3-6: 16384 rows, 8 per column.  The path beats the classic one -- with its one-pass panels -- by 1.4-3 x wherever its panels
// stay tall: tools/gpu_qr_shape_rule.py, 1024 x 256 fp64 2.04 -> 0.60 ms, 3000 x 512 1.95 -> 1.36 ms; with 3 rows per column the last
// panel still has 2 n + 64 rows)
static std::atomic<long> g_tq_min_rows{1024}, g_tq_min_aspect{3};
void tsqr_debug_shape_rule(long min_rows, long min_aspect)
{
	g_tq_min_rows.store(min_rows > 0 ? min_rows : 1024);
	g_tq_min_aspect.store(min_aspect > 0 ? min_aspect : 3);
}

static std::atomic<int> g_tq_f64{1};
void tsqr_debug_f64(int on) { g_tq_f64.store(on); }
static std::atomic<int> g_tq_panels{1};
void tsqr_debug_panels(int on) { g_tq_panels.store(on); }

template <typename T> bool tsqr_applicable(MatV<T> A, idx_t bs)
{
	const idx_t m = A.nrows, n = A.ncols;
	if (sizeof(T) == 8 && g_tq_f64.load() == 0)
		return false;
	// (columns that are not 16-byte aligned run the scalar-access variants of the streaming kernels)
	if (A.rs != 1 || A.cs < m || n < 1 || n > 512 || m < g_tq_min_rows.load() || m < g_tq_min_aspect.load() * n || m >= (1L << 30))
		return false;
	// T blocks are written per 64-column panel: a block of Q_coeff is either a whole number of panels or divides one
	return bs % TQ_PW == 0 || TQ_PW % bs == 0;
}
template bool tsqr_applicable<float>(MatV<float>, idx_t);
template bool tsqr_applicable<double>(MatV<double>, idx_t);

// Panels of the classic path (qr.hip, qr_rec): ONE panel of 16 .. 64 columns of a matrix of
// any shape, rows from its diagonal down, with its w x w block of T.  The one-pass panel costs a fixed ~180 us (Gram launch, reduce,
// the single-workgroup panel kernel, V launch, status read-back) against 9 us per column of the cooperative leaf + the level-3 steps
// of the recursion between 8 and 64 columns.
template <typename T> bool tsqr_panel_applicable(idx_t m, idx_t w, idx_t rs, idx_t cs)
{
	if (g_tq_panels.load() == 0 || (sizeof(T) == 8 && g_tq_f64.load() == 0))
		return false;
	// (ONE panel: any width up to 64 -- the block-size rule of tsqr_applicable is about panels that share a block of Q_coeff)
	// (... or a node of exactly two panels, 128 columns -- faer's block size of Q_coeff from N = 4096 on: one call, one read-back, the
	// first panel applied to the second by the path's own update launch, T12 from its small matrices)
	if (rs != 1 || cs < m || w < 16 || (w > TQ_PW && w != 2 * TQ_PW) || m < 256 || m < 4 * w || m >= (1L << 30))
		return false;
	// (the reference's rank test rejects every column of so tall a matrix: geqrf_classic, ref_rejects_all)
	return !(16.0 * (double) std::numeric_limits<T>::epsilon() * (double) m >= 1.0);
}
template bool tsqr_panel_applicable<float>(idx_t, idx_t, idx_t, idx_t);
template bool tsqr_panel_applicable<double>(idx_t, idx_t, idx_t, idx_t);

// ------------------------------------------------------------------------------------------------
// One call of either driver (tsqr_factor<float>: fused schedule; tsqr_factor<double>: plain schedule): the workspace, the
// launches in front of the first panel, the panel / y / cross-panel T launches and the status read-back.  The schedules stay in the drivers.
// ------------------------------------------------------------------------------------------------
template <typename T> struct TqWork {
	MatV<T> A, H;
	T *taus;
	idx_t m = A.nrows, n = A.ncols, ld = A.cs, bs = H.nrows;
	int npan = (int) ((n + TQ_PW - 1) / TQ_PW);
	int ldc = ((int) n + 63) & ~63, typ = ldc, ldz = ldc;
	hipStream_t s = ctx().stream;
	bool cross = bs > TQ_PW && npan > 1; // a block of Q_coeff spans several panels: cross-panel blocks of T
	// partial sums of the Gram launches: G (fp64), C and the column squares (scalar type)
	Scratch gp{(size_t) TQ_NB * 4096 * 8}, cp{(size_t) TQ_NB * 64 * TQ_TS * sizeof(T)}, sp{(size_t) TQ_NB * 256 * sizeof(T)};
	// fp64: G (NG x 4096), N1, N3, Gf (4096 each), C (NG x 64 x ldc), S (two slabs of NG x 256), abv (n + 64), Td, Md (npan x 4096 each),
	//       Z, B (npan x 64 x ldz each); then the scalar type: Mn (npan x 4096: V of step k may be formed beside panel k + 1), top, A1s
	//       (4096 each), Yn (64 x typ); then the status words
	Scratch small{((size_t) TQ_NG * 4096 + 3 * 4096 + (size_t) TQ_NG * 64 * ldc + (size_t) 2 * TQ_NG * 256 + (size_t) n + 64 + (size_t) 2 * npan * 4096 +
		       (size_t) 2 * npan * 64 * ldz) * 8 +
		      ((size_t) npan * 4096 + 2 * 4096 + (size_t) 64 * typ) * sizeof(T) + 2048};
	double *G, *N1, *N3, *Gf, *C, *S, *abv, *Td, *Md, *Z, *Bx;
	T *Mn, *top, *A1s, *Yn;
	int *stat;

	// zeroes the status words, abv and Z; the squares of the rows above the block (a panel of the classic path), the range guard of the
	// columns the first step's Gram launches do not cover
	TqWork(MatV<T> A_, MatV<T> H_, T *taus_, idx_t rows_above) : A(A_), H(H_), taus(taus_)
	{
		// (the streaming kernels load down the columns: tsqr_applicable / tsqr_panel_applicable admit nothing else)
		FH_CHECK(A.rs == 1, "tsqr: unit row stride");
		G = small.as<double>();
		N1 = G + (size_t) TQ_NG * 4096, N3 = N1 + 4096, Gf = N3 + 4096, C = Gf + 4096;
		S = C + (size_t) TQ_NG * 64 * ldc, abv = S + (size_t) 2 * TQ_NG * 256;
		Td = abv + n + 64, Md = Td + (size_t) npan * 4096, Z = Md + (size_t) npan * 4096, Bx = Z + (size_t) npan * 64 * ldz;
		Mn = reinterpret_cast<T *>(Bx + (size_t) npan * 64 * ldz), top = Mn + (size_t) npan * 4096, A1s = top + 4096, Yn = A1s + 4096;
		stat = reinterpret_cast<int *>(Yn + (size_t) 64 * typ);
		FH_HIP(hipMemsetAsync(stat, 0, 2048, s));
		FH_HIP(hipMemsetAsync(abv, 0, (size_t) (n + 64) * 8, s));
		if (rows_above > 0)
			hipLaunchKernelGGL(tq_above_kernel<T>, dim3((unsigned) n), dim3(256), 0, s, (const T *) A.p, (long) ld, (int) rows_above, abv);
		if (cross)
			FH_HIP(hipMemsetAsync(Z, 0, (size_t) npan * 64 * ldz * 8, s));
		if (n > TQ_PW + TQ_TS) {
			hipLaunchKernelGGL(tq_range_rest_kernel<T>, dim3((unsigned) (n - (TQ_PW + TQ_TS))), dim3(256), 0, s, A.p, (long) ld, (int) m, TQ_PW + TQ_TS, stat);
			FH_HIP(hipGetLastError());
		}
	}

	int width(int k) const { return (int) (n - k * TQ_PW < TQ_PW ? n - k * TQ_PW : TQ_PW); }

	// the panel kernel of panel k (one workgroup)
	void launch_panel(int k) const
	{
		const int c0 = k * TQ_PW, w = width(k), t = (int) n - c0 - w;
		TqPanelArgs<T> pa;
		pa.A = A.p;
		pa.ld = ld;
		pa.m = (int) m;
		pa.r0 = c0;
		pa.c0 = c0;
		pa.w = w;
		pa.n = (int) n;
		pa.G = Gf;
		pa.S = S;
		pa.check_range = k == 0;
		pa.range_cols = t < TQ_TS ? t : TQ_TS;
		pa.abv = abv;
		pa.N1 = N1;
		pa.N3 = N3;
		pa.Mn = Mn + (size_t) k * 4096;
		pa.top = top;
		pa.A1s = A1s;
		pa.Md = Md + (size_t) k * 4096;
		pa.Td = Td + (size_t) k * 4096;
		pa.H = H.p;
		pa.hrs = H.rs;
		pa.hcs = H.cs;
		pa.bs = (int) bs;
		pa.taus = taus;
		pa.stat = stat;
		pa.dbg = reinterpret_cast<long long *>(stat + 16);
		ProfScope prof(4, 1.0);
		hipLaunchKernelGGL(tq_panel_kernel<T>, dim3(1), dim3(TQ_PT), 0, s, pa);
	}

	// the y kernel of step k (Sr: the column squares its first launch checks), or behind the last panel the store of its top block
	void launch_y(int k, const double *Sr) const
	{
		const int c0 = k * TQ_PW, w = width(k), t = (int) n - c0 - w;
		if (t == 0) {
			hipLaunchKernelGGL(tq_top_kernel<T>, dim3(1), dim3(256), 0, s, A.p, (long) ld, c0, c0, w, (const T *) top, (const int *) stat);
			return;
		}
		TqYArgs<T> ya;
		ya.A = A.p;
		ya.ld = ld;
		ya.r0 = c0;
		ya.cx = c0 + w;
		ya.w = w;
		ya.t = t;
		ya.C = C;
		ya.ldc = ldc;
		ya.N1 = N1;
		ya.N3 = N3;
		ya.Md = Md + (size_t) k * 4096;
		ya.abv = abv;
		ya.Yn = Yn;
		ya.typ = typ;
		ya.Z = Z + (size_t) k * 64 * ldz;
		ya.ldz = ldz;
		ya.top = top;
		ya.stat = stat;
		ya.Sr = Sr;
		ya.check_range = k == 0;
		ya.range_cols = t < TQ_TS ? t : TQ_TS;
		ya.mrows = (int) m;
		hipLaunchKernelGGL(tq_y_kernel<T>, dim3((t + 15) / 16), dim3(256), 0, s, ya);
	}

	TqTxArgs<T> tx_args(int stage) const
	{
		TqTxArgs<T> ta;
		ta.A = A.p;
		ta.ld = ld;
		ta.n = (int) n;
		ta.bs = (int) bs;
		ta.Td = Td;
		ta.Md = Md;
		ta.Z = Z;
		ta.ldz = ldz;
		ta.B = Bx;
		ta.H = H.p;
		ta.hrs = H.rs;
		ta.hcs = H.cs;
		ta.stat = stat;
		ta.stage = stage;
		return ta;
	}

	// stage 1 or 2 of the cross-panel T blocks on the side stream, behind everything issued so far
	void launch_tx_stage(const TqSide &side, int stage) const
	{
		FH_HIP(hipEventRecord(side.xfork, s));
		FH_HIP(hipStreamWaitEvent(side.tx, side.xfork, 0));
		hipLaunchKernelGGL(tq_tx_kernel<T>, dim3(npan - 1), dim3(256), 0, side.tx, tx_args(stage));
	}

	// the cross-panel T blocks: the side stream's stages waited for (on_side), or formed now on the call's stream
	void finish_tx(const TqSide &side, bool on_side) const
	{
		if (!cross)
			return;
		if (on_side) {
			FH_HIP(hipEventRecord(side.xdone, side.tx));
			FH_HIP(hipStreamWaitEvent(s, side.xdone, 0));
		} else if (bs <= (TQ_TX_MAXL + 1) * TQ_PW) {
			hipLaunchKernelGGL(tq_tx_kernel<T>, dim3(npan - 1), dim3(256), 0, s, tx_args(0));
		} else {
			hipLaunchKernelGGL(tq_tx_general_kernel<T>, dim3(npan - 1), dim3(256), 0, s, tx_args(0));
		}
		FH_HIP(hipGetLastError());
	}

	// waits for the call's stream; the columns completed (n, or where a panel stopped it: *reason says why)
	idx_t columns_done(int *reason) const
	{
		int *st = ctx().pinned_ints(); // (a pageable target makes the copy a staged, blocking one)
		FH_HIP(hipMemcpyAsync(st, stat, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
#ifdef FH_TQ_TIMING
		{
			long long d[32];
			FH_HIP(hipMemcpy(d, stat + 16, sizeof(d), hipMemcpyDeviceToHost));
			fprintf(stderr, "tq_panel phases (shader cycles): start %lld: load %lld chol %lld reload %lld lu %lld finish %lld tests %lld out %lld M %lld T %lld\n",
				d[0], d[1] - d[0], d[2] - d[1], 0LL, d[3] - d[2], d[4] - d[3], d[5] - d[4], d[6] - d[5], d[7] - d[6], d[8] - d[7]);
			fprintf(stderr, "  load: range %lld loads %lld barrier %lld fill %lld | U, U^-1, V1^-1: %lld | A iterations:", d[12] - d[0], d[13] - d[12], d[14] - d[13], d[1] - d[14], d[15] - d[3]);
			for (int i = 0; i < 7; ++i)
				fprintf(stderr, " %lld", d[17 + i] - d[16 + i]);
			fprintf(stderr, " | B iterations:");
			for (int i = 0; i < 7; ++i)
				fprintf(stderr, " %lld", d[25 + i] - d[24 + i]);
			fprintf(stderr, "\n");
			double res[3];
			memcpy(res, d + 9, sizeof(res));
			fprintf(stderr, "tq_panel residuals of the last panel: |V1 V1^-1 - I| %.3e  |U U^-1 - I| %.3e  |R~ R~^-1 - I| %.3e\n", res[0], res[1], res[2]);
		}
#endif
		*reason = st[0] ? st[2] : TQ_OK;
		return st[0] ? (idx_t) st[1] : n;
	}
};

// Factors the leading panels of A (m x n fp32, column major) on the one-pass path.  Returns the number of COLUMNS
// completed (a multiple of 64, or n); the state is then that of the reference algorithm after those columns: R and
// V in place, the T blocks in H, taus[j] = T_jj, every reflector applied to all columns on the right.
// `reason` reports why it stopped early (TQ_FAIL_*).
template <> idx_t tsqr_factor<float>(MatV<float> A, MatV<float> H, float *taus, int *reason, idx_t rows_above)
{
	const TqWork<float> q(A, H, taus, rows_above);
	const idx_t m = q.m, n = q.n, ld = q.ld;
	const int npan = q.npan;
	hipStream_t s = q.s;
	const bool vec = (ld % 4 == 0) && ((uintptr_t) A.p % 16 == 0);
	const int ncu_all = ctx().stream_cus();
	int cus_taken = 0; // CUs held by side-stream kernels while the persistent update kernels run
	// two Gram workgroups per CU; a CU held by a side-stream kernel (its LDS leaves no room for one) would run its two AFTER the others
	auto gram_nb = [&]() { return cus_taken > 0 && ncu_all - cus_taken > 8 ? 2 * (ncu_all - cus_taken) : TQ_NB; };
	// Gram launches of panel [c0, c0 + w), rows from c0 down: G (want_g) and / or C against the columns [cx, cx + t) in strips
	// of <= 192
	auto launch_gram = [&](int c0, int w, bool want_g, int cx, int t, bool first, double *Sd) {
		const float *P = A.p + (long) c0 * ld + c0;
		const int rows = (int) (m - c0);
		if (t == 0) {
			if (want_g)
				tq_gram(P, P, ld, rows, w, 0, true, first, vec, q.gp.as<double>(), q.cp.as<float>(), q.sp.as<float>(), q.G, q.C, q.ldc, 0, Sd, q.stat, c0, q.A1s,
					q.Gf, q.stat + 128, gram_nb());
			return;
		}
		for (int off = 0; off < t; off += TQ_TS) {
			const int ts = t - off < TQ_TS ? t - off : TQ_TS;
			// the range guard of these launches covers the first strip only (n <= 256); tq_range_rest_kernel checks the others
			tq_gram(P, A.p + (long) (cx + off) * ld + c0, ld, rows, w, ts, want_g && off == 0, first && off == 0, vec, q.gp.as<double>(), q.cp.as<float>(),
				q.sp.as<float>(), q.G, q.C, q.ldc, cx + off - (c0 + w), Sd, q.stat, c0, q.A1s, q.Gf, q.stat + 128, gram_nb());
		}
	};
	// raw copy of the current panel below its top block for the U2 launches (see there); not for matrices where it would exceed 1 GiB
	const long ldpc = (long) ((m + 63) & ~(idx_t) 63);
	const bool want_copy = g_tq_panel_copy.load() != 0 && npan > 2 && (size_t) ldpc * TQ_PW * sizeof(float) <= ((size_t) 1 << 30);
	struct OptScratch {
		void *p = nullptr;
		~OptScratch()
		{
			if (p)
				ctx().release(p);
		}
		float *f() const { return static_cast<float *>(p); }
	} pcopy;
	if (want_copy)
		pcopy.p = ctx().alloc((size_t) ldpc * TQ_PW * sizeof(float));
	// one block of Q_coeff over all panels (the tall-skinny case): the cross-panel blocks of T in two stages beside the last steps
	const bool two_stage = q.cross && q.bs >= n && q.bs <= (TQ_TX_MAXL + 1) * TQ_PW && npan >= 2;
	// look-ahead: the columns of the next panel are updated first, its Gram matrix and its panel kernel (ONE workgroup, ~110 us)
	// follow at once, and the rest of the update + the products against the next panel run beside that kernel.  Variants that forced
	// it (always / a split Gram launch beside the panel kernel) measured slower and are gone: profiles/r03_qr_lookahead.txt keeps the record.
	const TqSide side = tq_side();
	bool tx_on_side = false;
	bool panel_on_side = false;
	double *Sy = q.S; // the column squares the first y kernel checks
	if (n > TQ_PW) {
		// the first panel's kernel needs G only: the products against the trailing columns (most of the first Gram launch: 190 us) run on
		// the side stream beside it; their column squares go to the second slab of S
		const int w0 = TQ_PW, t0 = (int) n - TQ_PW;
		launch_gram(0, w0, true, w0, 0, true, q.S);
		FH_HIP(hipEventRecord(side.pfork, s));
		FH_HIP(hipStreamWaitEvent(side.panel, side.pfork, 0));
		cus_taken += 1;
		{
			StreamScope sc(side.panel);
			Sy = q.S + (size_t) TQ_NG * 256;
			launch_gram(0, w0, false, w0, t0, true, Sy);
			FH_HIP(hipEventRecord(side.pdone, side.panel));
		}
		q.launch_panel(0);
		panel_on_side = true;
	} else {
		launch_gram(0, (int) n, true, (int) n, 0, true, q.S);
		q.launch_panel(0);
	}
	for (int k = 0; k < npan; ++k) {
		const int c0 = k * TQ_PW;
		const int w = q.width(k);
		const int t = (int) n - c0 - w;
		const int wn = t < TQ_PW ? t : TQ_PW; // width of the next panel
		if (panel_on_side) {
			FH_HIP(hipStreamWaitEvent(s, side.pdone, 0));
			panel_on_side = false;
			cus_taken -= 1;
		}
		q.launch_y(k, Sy);
		if (two_stage && k == npan - 1 && tx_on_side)
			q.launch_tx_stage(side, 2); // (it needs this panel's kernel and the V rows the last update wrote: beside the update below)
		const int r1 = c0 + w;
		const int rows = (int) (m - r1);
		const bool v2 = vec && r1 % 4 == 0;
		// V = P M as a launch of its own (it overwrites the panel); the side-stream kernels keep their CUs
		auto form_v = [&]() {
			if (rows <= 0)
				return;
			const TqFormVArgs va{A.p + (long) c0 * ld + r1, (long) ld, rows, w, q.Mn + (size_t) k * 4096, (rows + 127) / 128, q.stat, c0};
			tq_launch_form_v(v2, ncu_all - cus_taken > 8 ? ncu_all - cus_taken : ncu_all, va);
		};
		if (t > 0) {
			// ---- round 6: update + Gram in one pass, the next panel's kernel beside the second half
			const int nchunks = (rows + 63) / 64;
			TqFusedArgs fa;
			fa.P = A.p + (long) c0 * ld + r1;
			fa.N = A.p + (long) (c0 + w) * ld + r1;
			fa.F = fa.N;
			fa.ld = ld;
			fa.ldp = ld;
			fa.rows = rows;
			fa.w = w;
			fa.wn = wn;
			fa.ts = 0;
			fa.upd_n = 1;
			// V overwrites the panel, which the U2 launches read again: U1 leaves them a copy of the raw rows (one more write of 64
			// columns; a separate V launch behind U2 costs a read and a write and ran beside the next step's first kernels: the y kernel
			// 17 -> 80 us, U1 114 -> 180 us)
			const bool copyp = t - wn > 0 && pcopy.p;
			fa.do_v = t - wn == 0 || copyp;
			fa.Pc = copyp ? pcopy.f() : nullptr;
			fa.ldpc = ldpc;
			fa.want_g = 1;
			fa.Yn = q.Yn;
			fa.typ = q.typ;
			fa.fo = 0;
			fa.Mn = q.Mn + (size_t) k * 4096;
			fa.Gp = q.gp.as<double>();
			fa.Cp = q.cp.as<float>();
			fa.tp = 0;
			fa.nchunks = nchunks;
			fa.A1s = q.A1s;
			fa.stat = q.stat;
			fa.c0 = c0;
			auto grid = [&]() { // two workgroups per CU
				const int ncu = ncu_all - cus_taken > 8 ? ncu_all - cus_taken : ncu_all;
				return nchunks < 2 * ncu ? nchunks : 2 * ncu;
			};
			const int nc0 = c0 + w; // first column of the next panel
			// U1: the next panel's columns, its Gram matrix, V = P M
			int nb = grid();
			tq_launch_fused(v2, 1, nb, fa);
			hipLaunchKernelGGL(tq_reduce_kernel<float>, dim3(4096 / 256, TQ_NG), dim3(256), 0, s, fa.Gp, fa.Cp, q.sp.as<float>(), nb, 0, 1, 0, q.G, q.C, q.ldc, 0, q.S, q.stat, nc0,
					   q.Gf, q.stat + 128);
			if (t - wn > 0) {
				// U2 (side stream): the columns behind it and C'; the next panel's kernel runs on the main stream meanwhile
				FH_HIP(hipEventRecord(side.pfork, s));
				FH_HIP(hipStreamWaitEvent(side.panel, side.pfork, 0));
				cus_taken += 1;
				{
					StreamScope sc(side.panel);
					fa.upd_n = 0;
					fa.want_g = 0;
					fa.do_v = 0;
					if (copyp) {
						fa.P = pcopy.f();
						fa.ldp = ldpc;
					}
					for (int fo = 0; fo < t - wn; fo += TU_CF) {
						fa.ts = t - wn - fo < TU_CF ? t - wn - fo : TU_CF;
						fa.tp = (fa.ts + 31) & ~31;
						fa.fo = fo;
						fa.F = A.p + (long) (nc0 + wn + fo) * ld + r1;
						nb = grid();
						tq_launch_fused(v2, 2, nb, fa);
						hipLaunchKernelGGL(tq_reduce_kernel<float>, dim3((64 * fa.tp + 255) / 256, TQ_NG), dim3(256), 0, side.panel, fa.Gp, fa.Cp, q.sp.as<float>(), nb,
								   fa.tp, 0, 0, q.G, q.C, q.ldc, fo, q.S, q.stat, nc0, q.Gf, q.stat + 128);
					}
					FH_HIP(hipEventRecord(side.pdone, side.panel));
					// V = P M once nothing reads the panel any more: behind U2 on the side stream, beside the next step's first
					// launches (nothing waits for it before the end of the factorization or the cross-panel T blocks)
					// (only without the raw copy: matrices too tall for it)
					if (!copyp)
						form_v();
				}
				panel_on_side = true; // (here: U2 is what runs on the side stream)
			}
			// everything of the cross-panel T blocks that does not depend on the last panel's kernel: beside the Gram / reduce / panel
			// kernels of the last panel (a single workgroup busy most of that time), one CU per panel.  The fork is recorded BEHIND the
			// update of step npan - 2 and IN FRONT of the last panel's launches (rounds 3-5 recorded it behind them: the stage then ran
			// beside the last update and the factorization ended with ~110 us of three workgroups)
			if (two_stage && k == npan - 2) {
				q.launch_tx_stage(side, 1);
				tx_on_side = true;
				if (ncu_all > 8 * npan)
					cus_taken += npan - 1;
			}
			q.launch_panel(k + 1);
		} else {
			form_v();
		}
		FH_HIP(hipGetLastError());
	}
	q.finish_tx(side, tx_on_side);
	if (npan > 1) { // the V launches on the side stream
		FH_HIP(hipEventRecord(side.pdone, side.panel));
		FH_HIP(hipStreamWaitEvent(s, side.pdone, 0));
	}
	return q.columns_done(reason);
}

// ------------------------------------------------------------------------------------------------
// fp64 driver: the contract of tsqr_factor for double data (columns completed, state of the reference algorithm at that column)
// ------------------------------------------------------------------------------------------------
// the plain schedule: Gram, panel, y, update per panel on one stream
template <> idx_t tsqr_factor<double>(MatV<double> A, MatV<double> H, double *taus, int *reason, idx_t rows_above)
{
	const TqWork<double> q(A, H, taus, rows_above);
	const idx_t m = q.m, n = q.n, ld = q.ld;
	const int npan = q.npan;
	hipStream_t s = q.s;
	constexpr int RPV = TqVec<double>::RPV;
	// 16-byte accesses down the columns where they are aligned (faer's Mat pads the column stride to 64 bytes; a view that starts at an odd
	// row or has an odd column stride runs the same kernels with scalar accesses)
	const bool vec = ld % RPV == 0 && (uintptr_t) A.p % 16 == 0;
	const int ncu = ctx().stream_cus();
	// Gram launches of panel [c0, c0 + w), rows from c0 down, against the columns [cx, cx + t) in strips of <= 192
	auto launch_gram = [&](int c0, int w, int cx, int t, bool first) {
		const int rows = (int) (m - c0);
		const int nstrip = t == 0 ? 1 : (t + TQ_TS - 1) / TQ_TS;
		for (int st = 0; st < nstrip; ++st) {
			const int off = st * TQ_TS;
			TqGramTArgs<double> g;
			g.P = A.p + (long) c0 * ld + c0;
			g.X = A.p + (long) (cx + off) * ld + c0;
			g.ld = ld;
			g.rows = rows;
			g.w = w;
			g.t = t - off < TQ_TS ? t - off : TQ_TS;
			g.tp = (g.t + 63) & ~63;
			{
				const int nslot = (TQ_PW + g.tp + 63) / 64;
				g.nsub = 4 / nslot;
			}
			g.nchunks = (rows + 8 * RPV * g.nsub - 1) / (8 * RPV * g.nsub);
			g.want_g = st == 0;
			g.want_sq = first && st == 0; // (the range guard covers the first strip; tq_range_rest_kernel checks the others)
			g.Gp = q.gp.as<double>();
			g.Cp = q.cp.as<double>();
			g.Sp = q.sp.as<double>();
			g.stat = q.stat;
			g.c0 = c0;
			g.A1s = q.A1s;
			const int nb = g.nchunks < ncu ? g.nchunks : ncu; // one persistent workgroup per CU (<= TQ_NB partial sums)
			{
				ProfScope prof(3, (double) rows * 8.0 * ((double) w + (double) g.t));
				switch (g.tp / 32) {
				case 0: if (vec)
						hipLaunchKernelGGL((tq_gramT_kernel<double, 0, true>), dim3(nb), dim3(512), 0, s, g);
					else
						hipLaunchKernelGGL((tq_gramT_kernel<double, 0, false>), dim3(nb), dim3(512), 0, s, g); break;
				case 2: if (vec)
						hipLaunchKernelGGL((tq_gramT_kernel<double, 2, true>), dim3(nb), dim3(512), 0, s, g);
					else
						hipLaunchKernelGGL((tq_gramT_kernel<double, 2, false>), dim3(nb), dim3(512), 0, s, g); break;
				case 4: if (vec)
						hipLaunchKernelGGL((tq_gramT_kernel<double, 4, true>), dim3(nb), dim3(512), 0, s, g);
					else
						hipLaunchKernelGGL((tq_gramT_kernel<double, 4, false>), dim3(nb), dim3(512), 0, s, g); break;
				default: if (vec)
						hipLaunchKernelGGL((tq_gramT_kernel<double, 6, true>), dim3(nb), dim3(512), 0, s, g);
					else
						hipLaunchKernelGGL((tq_gramT_kernel<double, 6, false>), dim3(nb), dim3(512), 0, s, g); break;
				}
			}
			const int total = (g.want_g ? 4096 : 0) + 64 * g.tp + (g.want_sq ? 256 : 0);
			hipLaunchKernelGGL(tq_reduce_kernel<double>, dim3((total + 255) / 256, TQ_NG), dim3(256), 0, s, g.Gp, g.Cp, g.Sp, nb, g.tp, g.want_g, g.want_sq, q.G, q.C, q.ldc,
					   cx + off - (c0 + w), q.S, q.stat, c0, q.Gf, q.stat + 128);
			FH_HIP(hipGetLastError());
		}
	};
	// one block of Q_coeff over all panels (the tall-skinny case): the cross-panel blocks of T in two stages on the side stream -- what
	// does not need the last panel's kernel beside that panel's Gram launch and kernel, the rest beside the last update (tsqr_factor)
	const bool two_stage = q.cross && q.bs >= n && q.bs <= (TQ_TX_MAXL + 1) * TQ_PW && npan >= 2;
	const TqSide side = tq_side();
	for (int k = 0; k < npan; ++k) {
		const int c0 = k * TQ_PW;
		const int w = q.width(k);
		const int t = (int) n - c0 - w;
		if (two_stage && k == npan - 1)
			q.launch_tx_stage(side, 1);
		launch_gram(c0, w, c0 + w, t, k == 0);
		q.launch_panel(k);
		q.launch_y(k, q.S);
		if (two_stage && k == npan - 1)
			q.launch_tx_stage(side, 2); // (it reads this panel's R block and M: beside the update below, which writes V below that block only)
		const int r1 = c0 + w;
		const int rows = (int) (m - r1);
		if (rows > 0) {
			TqUpdTArgs<double> ua;
			ua.P = A.p + (long) c0 * ld + r1;
			ua.ld = ld;
			ua.rows = rows;
			ua.w = w;
			ua.Yn = q.Yn;
			ua.typ = q.typ;
			ua.Mn = q.Mn + (size_t) k * 4096;
			ua.nchunks = (rows + 16 * RPV - 1) / (16 * RPV);
			ua.stat = q.stat;
			ua.c0 = c0;
			const bool v2 = vec && r1 % RPV == 0;
			const int nwg = ua.nchunks < ncu ? ua.nchunks : ncu; // one persistent 512-thread workgroup per CU
			// strips of at most 192 columns; V = P M (it overwrites the panel) rides on the last one
			int from = 0;
			do {
				int ts = t - from;
				const bool last = ts <= TQ_TS;
				if (!last)
					ts = TQ_TS;
				ua.coff = from;
				ua.ts = ts;
				ua.X = A.p + (long) (c0 + w + from) * ld + r1;
				ua.do_v = last;
				ProfScope prof(2, (double) rows * 8.0 * ((double) w + 2.0 * (double) ts + (last ? (double) w : 0.0)));
				if (v2)
					hipLaunchKernelGGL((tq_updateT_kernel<double, true>), dim3(nwg), dim3(512), 0, s, ua);
				else
					hipLaunchKernelGGL((tq_updateT_kernel<double, false>), dim3(nwg), dim3(512), 0, s, ua);
				from += ts;
				if (last)
					break;
			} while (true);
		}
		FH_HIP(hipGetLastError());
	}
	q.finish_tx(side, two_stage);
	return q.columns_done(reason);
}

} // namespace fh
