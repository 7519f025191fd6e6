// Reductions to condensed form for gfx950: tridiagonalization of a self-adjoint matrix (tridiag_dev), bidiagonalization
// (bidiag_dev) and Hessenberg reduction (hessenberg_dev).  Three level-2, HBM-bound algorithms that follow the reference's
// unblocked variants column by column; each section below opens with its own description.  They share the launch shape of
// their vector kernels, the tiles of their fused passes, the wavefront helpers of those passes and the reflector of a column.
#include <atomic>
#include <limits>

#include "common.h"
#include "reduce.h"
#include "xwg.h"

namespace fh {

// ------------------------------------------------------------------------------------------------
// shared by the three reductions
// ------------------------------------------------------------------------------------------------
// tests: 1 = the vector kernels of the three reductions run their memory-resident bodies at every size (the bodies that keep their columns
// in registers take over from 4096 remaining rows down)
static std::atomic<int> g_l2_force_mem{0};
void level2_debug_force_memory_bodies(int on) { g_l2_force_mem.store(on); }

constexpr int LV2_NT = 1024; // threads of the vector kernels (td_step_kernel, bd_pre_kernel, bd_mid_kernel, hs_pre_kernel)
constexpr int LV2_E = 4;    // entries per thread and vector of their register-resident bodies (at most LV2_E LV2_NT remaining rows)
constexpr int TF_TR = 128;  // rows of a tile of the fused pass
constexpr int TF_TC = 64;   // columns of a tile = entries of an index block
constexpr int TF_NT = 256;  // its threads: wavefront w owns 16 columns of the tile, a lane two rows

// value of lane `l` (compile-time after unrolling) for the whole wavefront
static __device__ __forceinline__ double lv2_lane(double v, int l)
{
	const long long b = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_readlane((int) b, l), hi = __builtin_amdgcn_readlane((int) (b >> 32), l);
	return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
}
static __device__ __forceinline__ float lv2_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// sum over the wavefront, uniform: butterflies inside the rows of 16 lanes on the DPP path (xor 1, xor 2, half mirror, mirror), then
// the four row sums in a fixed order (the __shfl_xor form goes through the LDS crossbar: 12 ds_bpermute per sum)
template <int CTRL> static __device__ __forceinline__ double lv2_dpp(double v)
{
	const long long b = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_update_dpp(0, (int) b, CTRL, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, (int) (b >> 32), CTRL, 0xf, 0xf, true);
	return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
}
static __device__ __forceinline__ double lv2_wave_sum(double v)
{
	v += lv2_dpp<0xB1>(v);  // quad_perm [1, 0, 3, 2]
	v += lv2_dpp<0x4E>(v);  // quad_perm [2, 3, 0, 1]
	v += lv2_dpp<0x141>(v); // row_half_mirror
	v += lv2_dpp<0x140>(v); // row_mirror
	return ((lv2_lane(v, 0) + lv2_lane(v, 16)) + lv2_lane(v, 32)) + lv2_lane(v, 48);
}

// make_householder_imp (householder.rs:59-107) from the head and the scaled sums of the tail; returns tau, sets
// head <- beta, hinv (0 if the tail is negligible: nothing is scaled), inf_flag
template <typename T> static __device__ __forceinline__ T lv2_householder(T &head, T tail_norm, T &hinv, bool &negligible)
{
	T head_norm = fabs(head);
	if (head_norm < Lim<T>::minpos) {
		head = (T) 0;
		head_norm = (T) 0;
	}
	negligible = tail_norm < Lim<T>::minpos;
	hinv = (T) 0;
	if (negligible)
		return std::numeric_limits<T>::infinity();
	const T norm = (T) hypot((double) head_norm, (double) tail_norm);
	const T sign = head_norm != (T) 0 ? head * ((T) 1 / head_norm) : (T) 1;
	const T signed_norm = sign * norm;
	hinv = (T) 1 / (head + signed_norm);
	head = -signed_norm;
	const T tn = tail_norm * fabs(hinv);
	return (T) 0.5 * ((T) 1 + tn * tn);
}

// one entry more in the three scaled sums of squares of a norm (reductions/norm_l2.rs:6-45).  A macro: as an inline function the same three
// statements make the compiler pack the fp32 products of the vector kernels differently
#define LV2_NORM_ACC(acc, v, sml, big) \
	do { \
		(acc)[0] += ((v) * (sml)) * ((v) * (sml)); \
		(acc)[1] += (v) * (v); \
		(acc)[2] += ((v) * (big)) * ((v) * (big)); \
	} while (0)

// the sum of the `np` shares src[p * stride] in the order of p, eight loads in flight
static __device__ __forceinline__ double lv2_sum_shares(const double *src, const int np, const size_t stride)
{
	double s0 = 0.0;
	int p = 0;
	for (; p + 8 <= np; p += 8) {
		double v[8];
#pragma unroll
		for (int u = 0; u < 8; ++u)
			v[u] = src[(size_t) (p + u) * stride];
#pragma unroll
		for (int u = 0; u < 8; ++u)
			s0 += v[u];
	}
	for (; p < np; ++p)
		s0 += src[(size_t) p * stride];
	return s0;
}

// end of a helper block of a vector kernel: its write-through stores have left, then ONE flag tells block 0 of the same launch (xwg.h)
static __device__ __forceinline__ void lv2_helper_done(xwg_u64 *flag, const xwg_u64 epoch)
{
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if (threadIdx.x == 0)
		__hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// Tridiagonalization of a self-adjoint matrix -- faer/src/linalg/evd/tridiag.rs:274-535.
// A level-2, HBM-bound algorithm like the reference's: per column ONE pass over the remaining lower triangle that
// applies the symmetric rank-2 update of the previous reflector and multiplies the updated matrix by the new one
// (tridiag_fused_op, :36-272), between two short vector phases.  Two launches per column, no host synchronisation:
//   td_step_kernel(k)   block 0: finishes y of step k-1 (:484-511), brings column k up to date (:300-318), makes its reflector
//                       (:330-336, householder.rs:59-107), updates column k+1 (:348-359), w <- y; blocks 1 ..: add the shares of the
//                       previous pass in a fixed order -> ysum (one block per 64 entries) while block 0 loads its columns, and hand
//                       them over inside the launch (write-through stores + one flag per block, xwg.h: no fence)
//   td_fused_kernel(k)  one workgroup per 128 x 64 tile of the lower triangle of A22 = A[k+2.., k+2..], lanes along the rows:
//                       A22 -= u w^H + w u^H written back (every entry is read and written ONCE) and the tile's share of both halves
//                       of sym(A22) x -- the row sums tril(A22) x and the column sums striu(A22^H) x
// History (N = 4096 fp64): rounds 2-5 read the triangle twice (a column pass that wrote back and a 16-row pass, each sum complete in
// one wavefront / workgroup): 185 ms; cut into uniform pieces with partial sums added by the step kernel: 150 ms (the chip had waited
// for the longest workgroup); one pass over tiles, the sums inside that pass behind an arrival counter (write-through + atomic, no fence): 140 ms
// -- the tail "drain, count, reload, add" is four memory round trips in every launch; the sums as a launch of their own: 116 ms; loads
// without branches, DPP column sums, a step kernel that holds its three columns in registers: 95 ms; the sums as helper blocks of the
// step launch: 88 ms.  Running the vector phase in the last workgroup behind a release fence measured 2.4x slower in round 2 (an
// agent-scope fence writes the L2 back).
// ------------------------------------------------------------------------------------------------
struct TdState {
	double tau_inv;
};
template <typename T> struct TdArgs {
	T *A;
	idx_t rs, cs;
	int n, k, force_mem;
	T *y, *w, *taus;
	double *ysum;	       // sym(A22) x of the fused pass, complete
	double *rpart, *cpart; // shares of the tiles: row sums rpart[J * n + i] (column block J), column sums cpart[I * n + j] (row block I)
	xwg_u64 *flags;	       // per index block: the step whose sums are complete (td_sum_block / td_wait_sums)
	TdState *st;
};

// Tiles of the lower triangle of an r x r matrix, TF_TR rows x TF_TC columns: tile (I, J) exists for J <= 2 I + 1 and J < ncb; row block I has
// td_row_tiles(I) of them, column block J lives in the row blocks J / 2 .. nbr - 1.
static __device__ __forceinline__ int td_row_tiles(int I, int ncb) { return min(2 * I + 2, ncb); }

// Index block b of TF_TC entries of the fused pass of step kk (A22 = A[kk+2.., kk+2..]): the shares of its row tiles and of its column's
// tiles, added in a fixed order -> ysum, by the 1024 threads of the calling workgroup; stored write-through (xwg.h) because the reader is
// another workgroup of the SAME launch: the blocks 1 .. of td_step_kernel(k) add the shares of pass k - 1 while block 0 loads its columns,
// then raise their flag; block 0 waits for the flags and reads the sums past its caches.  (A launch of its own for the sums -- round 6's
// first version -- cost 4.7 us per column: a launch and a memory round trip that nothing overlapped.)
constexpr int TS_NT = 1024, TS_NS = TS_NT / TF_TC; // 16 slices of the list of shares per entry
template <typename T> static __device__ __forceinline__ void td_sum_block(const TdArgs<T> &a, const int kk, const int b)
{
	__shared__ double s_q[TS_NS][TF_TC];
	const int tid = threadIdx.x;
	const int base = kk + 2, r = a.n - base;
	const int nbr = (r + TF_TR - 1) / TF_TR, ncb = (r + TF_TC - 1) / TF_TC;
	const int Ib = b >> 1;
	const int nrp = td_row_tiles(Ib, ncb), tot = nrp + (nbr - Ib);
	const int e = tid & 63, qq = tid >> 6, i = min(b * TF_TC + e, r - 1);
	const int per = (tot + TS_NS - 1) / TS_NS, p0 = qq * per;
	double sacc = 0.0;
	for (int pb = 0; pb < per; pb += 4) {
		double v[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) {
			const int p = p0 + pb + u;
			const bool in = pb + u < per && p < tot;
			const int pc = in ? p : 0;
			const double *src = pc < nrp ? a.rpart + (size_t) pc * a.n : a.cpart + (size_t) (Ib + pc - nrp) * a.n;
			v[u] = src[base + i];
			if (!in)
				v[u] = 0.0;
		}
		sacc += (v[0] + v[1]) + (v[2] + v[3]);
	}
	__syncthreads(); // (s_q of a previous call has been read)
	s_q[qq][e] = sacc;
	__syncthreads();
	if (tid < TF_TC && b * TF_TC + tid < r) {
		double t = 0.0;
#pragma unroll
		for (int q = 0; q < TS_NS; ++q)
			t += s_q[q][tid];
		xwg_store(a.ysum + base + b * TF_TC + tid, t);
	}
}
// block 0 of td_step_kernel(k), k > 0: the sums of pass k - 1 are complete (flags of the helper blocks; if they do not come -- the
// launch shares the GPU and the helpers are not resident -- block 0 adds the shares itself)
template <typename T> static __device__ __forceinline__ void td_wait_sums(const TdArgs<T> &a, const int k)
{
	__shared__ int s_flag;
	const int nsb = (a.n - (k + 1) + TF_TC - 1) / TF_TC;
	if (nsb <= 0)
		return;
	if (!xwg_wait_all(a.flags, nsb, (xwg_u64) k, &s_flag)) {
		for (int b = 0; b < nsb; ++b)
			td_sum_block<T>(a, k - 1, b);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
	}
}

template <typename T> static __device__ __forceinline__ void td_step_body(const TdArgs<T> &a, const int k)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	const int tid = threadIdx.x, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	T nacc[3] = {0, 0, 0}; // scaled sums of the tail of column k (reductions/norm_l2.rs:6-45)
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	if (k > 0) {
		// ---- y of step k - 1 (:484-511): x = the reflector in column k-1 (rows k+1..), ysum = sym(A22) x from the fused pass
		const T tau_inv = (T) a.st->tau_inv;
		td_wait_sums<T>(a, k);
		double d[2] = {0.0, 0.0};
		for (int i = k + 1 + tid; i < n; i += LV2_NT) {
			const T aik = at(i, k), xi = at(i, k - 1);
			T yv = tau_inv * (T) xwg_load(a.ysum + i);
			yv += aik * tau_inv;
			a.y[i] = yv;
			d[0] += (double) aik * (double) xi;
			d[1] += (double) xi * (double) yv;
		}
		block_sum<LV2_NT, 2>(d, s_part, s_red);
		T y1 = (at(k, k) + (T) s_red[0]) * tau_inv;
		const T b = ((y1 + (T) s_red[1]) * (T) 0.5) * tau_inv;
		y1 -= b;
		__syncthreads(); // at(k, k) was read by everyone
		// ---- y -= b x, then column k receives the rest of the rank-2 update (:300-318), norm of its tail on the way
		for (int i = k + 1 + tid; i < n; i += LV2_NT) {
			const T xi = at(i, k - 1);
			const T yi = a.y[i] - b * xi;
			a.y[i] = yi;
			const T v = at(i, k) - (y1 * xi + yi);
			at(i, k) = v;
			if (i >= k + 2) {
				LV2_NORM_ACC(nacc, v, sml, big);
			}
		}
		if (tid == 0) {
			a.y[k] = y1;
			at(k, k) -= y1 + y1;
		}
	} else {
		for (int i = 2 + tid; i < n; i += LV2_NT) {
			const T v = at(i, 0);
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	}
	if (k + 1 >= n)
		return;
	// ---- reflector of column k below the diagonal (:330-336)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red); // (its barriers also publish the column written above)
	const T tail_norm = norm_from3<T>(s_red);
	T head = at(k + 1, k), hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	const bool scale_tail = !negligible;
	__syncthreads(); // everyone has read the old head
	const T u1 = k > 0 ? at(k + 1, k - 1) : (T) 0, y1n = k > 0 ? a.y[k + 1] : (T) 0;
	for (int i = k + 2 + tid; i < n; i += LV2_NT) {
		if (scale_tail)
			at(i, k) *= hinv;
		if (k > 0) { // :348-359
			const T yi = a.y[i];
			at(i, k + 1) -= at(i, k - 1) * y1n + yi * u1;
			a.w[i] = yi;
		}
	}
	if (tid == 0) {
		at(k + 1, k) = head;
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		if (k > 0)
			at(k + 1, k + 1) -= u1 * y1n + y1n * u1;
	}
}

// The same step with every entry of the three columns it touches held in registers (at most LV2_E rows per thread: n - k - 1 <= LV2_E LV2_NT):
// all loads are issued at the start -- ONE round trip to memory instead of one per loop -- and every entry is stored once.  Same arithmetic,
// expression by expression, as td_step_body.
template <typename T> static __device__ __forceinline__ void td_step_body_reg(const TdArgs<T> &a, const int k)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	__shared__ T s_bc[3];
	const int tid = threadIdx.x, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const bool upd = k > 0, more = k + 1 < n;
	// rows i = k + 1 + tid + e LV2_NT: column k (aik), the previous reflector (xi), column k + 1 (ak1), the product of the fused pass (ys)
	T aik[LV2_E], xi[LV2_E], ak1[LV2_E], yi[LV2_E];
	double ys[LV2_E];
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + 1 + tid + e * LV2_NT;
		const bool in = i < n;
		const int ic = in ? i : n - 1;
		aik[e] = at(ic, k);
		xi[e] = upd ? at(ic, k - 1) : (T) 0;
		ys[e] = 0.0;
		ak1[e] = (upd && more) ? at(ic, k + 1) : (T) 0;
		yi[e] = (T) 0;
	}
	const T akk = at(k, k), tau_inv = (T) a.st->tau_inv;
	if (upd) { // (the loads above are in flight while the helper blocks finish the sums)
		td_wait_sums<T>(a, k);
#pragma unroll
		for (int e = 0; e < LV2_E; ++e) {
			const int i = k + 1 + tid + e * LV2_NT;
			ys[e] = xwg_load(a.ysum + (i < n ? i : n - 1));
		}
	}
	T y1 = (T) 0;
	T nacc[3] = {0, 0, 0}; // scaled sums of the tail of column k (reductions/norm_l2.rs:6-45)
	if (upd) {
		// ---- y of step k - 1 (:484-511)
		double d[2] = {0.0, 0.0};
#pragma unroll
		for (int e = 0; e < LV2_E; ++e)
			if (k + 1 + tid + e * LV2_NT < n) {
				T yv = tau_inv * (T) ys[e];
				yv += aik[e] * tau_inv;
				yi[e] = yv;
				d[0] += (double) aik[e] * (double) xi[e];
				d[1] += (double) xi[e] * (double) yv;
			}
		block_sum<LV2_NT, 2>(d, s_part, s_red);
		y1 = (akk + (T) s_red[0]) * tau_inv;
		const T b = ((y1 + (T) s_red[1]) * (T) 0.5) * tau_inv;
		y1 -= b;
		// ---- y -= b x, then column k receives the rest of the rank-2 update (:300-318), norm of its tail on the way
#pragma unroll
		for (int e = 0; e < LV2_E; ++e) {
			const int i = k + 1 + tid + e * LV2_NT;
			if (i < n) {
				yi[e] -= b * xi[e];
				aik[e] -= y1 * xi[e] + yi[e];
			}
		}
	}
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + 1 + tid + e * LV2_NT;
		if (i < n && i >= k + 2) {
			const T v = aik[e];
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	}
	if (tid == 0 && upd)
		at(k, k) = akk - (y1 + y1);
	if (!more)
		return;
	if (tid == 0) { // row k + 1: the head of the column, y and u of the update of column k + 1
		s_bc[0] = aik[0];
		s_bc[1] = yi[0];
		s_bc[2] = xi[0];
	}
	// ---- reflector of column k below the diagonal (:330-336)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = s_bc[0], hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	const bool scale_tail = !negligible;
	const T u1 = upd ? s_bc[2] : (T) 0, y1n = upd ? s_bc[1] : (T) 0;
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + 1 + tid + e * LV2_NT;
		if (i < n && i >= k + 2) {
			if (scale_tail || upd)
				at(i, k) = scale_tail ? aik[e] * hinv : aik[e];
			if (upd) { // :348-359
				at(i, k + 1) = ak1[e] - (xi[e] * y1n + yi[e] * u1);
				a.w[i] = yi[e];
			}
		}
	}
	if (tid == 0) {
		at(k + 1, k) = head;
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		if (upd)
			at(k + 1, k + 1) = ak1[0] - (u1 * y1n + y1n * u1);
	}
}

template <typename T> __global__ __launch_bounds__(LV2_NT) void td_step_kernel(const TdArgs<T> a)
{
	if (blockIdx.x > 0) { // helper block: the sums of index block blockIdx.x - 1 of pass k - 1
		td_sum_block<T>(a, a.k - 1, (int) blockIdx.x - 1);
		lv2_helper_done(a.flags + (blockIdx.x - 1), (xwg_u64) a.k);
		return;
	}
	if (a.n - a.k - 1 <= LV2_E * LV2_NT && !a.force_mem)
		td_step_body_reg<T>(a, a.k);
	else
		td_step_body<T>(a, a.k);
}

// Tile (I, J) of A22 (header of this section).  Lane l of wavefront w: rows 128 I + l and + 64, columns 64 J + 16 w .. + 15; all 32 loads
// of a thread are issued before the first use.
template <typename T, bool upd> __global__ __launch_bounds__(TF_NT) void td_fused_kernel(const TdArgs<T> a)
{
	constexpr int CW = TF_TC / (TF_NT / 64); // 16 columns per wavefront
	__shared__ double s_row[TF_NT / 64][TF_TR];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k;
	const int base = k + 2, r = a.n - base; // A22 = A[base.., base..], r x r
	const int nbr = (r + TF_TR - 1) / TF_TR, ncb = (r + TF_TC - 1) / TF_TC;
	const int t = blockIdx.x; // tile (I, J): t in [I (I + 1), (I + 1)(I + 2))
	int I = (int) ((sqrtf(4.0f * (float) t + 1.0f) - 1.0f) * 0.5f);
	while (I * (I + 1) > t)
		--I;
	while ((I + 1) * (I + 2) <= t)
		++I;
	const int J = t - I * (I + 1);
	if (J >= ncb)
		return;
	const T *u = a.A + (idx_t) base * a.rs + (idx_t) (upd ? k - 1 : 0) * a.cs; // u[i * rs]
	const T *x = a.A + (idx_t) base * a.rs + (idx_t) k * a.cs;
	const T *w = a.w + base;
	T *A22 = a.A + (idx_t) base * a.rs + (idx_t) base * a.cs;
	const int i0 = I * TF_TR, j0 = J * TF_TC + CW * wv;
	int gi[2];
	bool vr[2];
	T xi[2], ui[2], wi[2];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		gi[h] = i0 + lane + 64 * h;
		vr[h] = gi[h] < r;
		gi[h] = min(gi[h], r - 1); // (loads below are unconditional: a row past the end reads the last row and takes part in nothing)
		const idx_t o = (idx_t) gi[h] * a.rs;
		xi[h] = x[o];
		ui[h] = upd ? u[o] : (T) 0;
		wi[h] = upd ? w[gi[h]] : (T) 0;
	}
	T xjl, ujl, wjl; // column values of the wavefront's 16 columns, one per lane
	{
		const int gj = min(j0 + (lane & (CW - 1)), r - 1);
		const idx_t o = (idx_t) gj * a.rs;
		xjl = x[o];
		ujl = upd ? u[o] : (T) 0;
		wjl = upd ? w[gj] : (T) 0;
	}
	T v[2][CW];
#pragma unroll
	for (int c = 0; c < CW; ++c)
#pragma unroll
		for (int h = 0; h < 2; ++h) // an entry above the diagonal reads the diagonal entry of its row instead (and is not used)
			v[h][c] = A22[(idx_t) gi[h] * a.rs + (idx_t) min(j0 + c, gi[h]) * a.cs];
	double racc[2] = {0.0, 0.0};
#pragma unroll
	for (int c = 0; c < CW; ++c) {
		const int gj = j0 + c;
		const T xj = lv2_lane(xjl, c), uj = lv2_lane(ujl, c), wj = lv2_lane(wjl, c);
		double cs_ = 0.0;
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const bool in = vr[h] && gj <= gi[h];
			T tv = v[h][c];
			if (upd) {
				tv = fh_fma(-ui[h], wj, tv);
				tv = fh_fma(-wi[h], uj, tv);
				if (in)
					A22[(idx_t) gi[h] * a.rs + (idx_t) gj * a.cs] = tv;
			}
			racc[h] += in ? (double) tv * (double) xj : 0.0;
			cs_ += (in && gj < gi[h]) ? (double) tv * (double) xi[h] : 0.0; // the diagonal entry is not part of the strictly-upper product
		}
		const double sv = lv2_wave_sum(cs_);
		if (lane == 0 && gj < r)
			a.cpart[(size_t) I * a.n + base + gj] = sv;
	}
	s_row[wv][lane] = racc[0];
	s_row[wv][lane + 64] = racc[1];
	__syncthreads();
	if (tid < TF_TR && i0 + tid < r)
		a.rpart[(size_t) J * a.n + base + i0 + tid] = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
}

// A: n x n (lower triangle used), H: block_size x (n - 1)
template <typename T> void tridiag_dev(MatV<T> A, MatV<T> H)
{
	const idx_t n = A.nrows;
	FH_CHECK(A.ncols == n, "tridiag: the matrix must be square");
	FH_CHECK(H.nrows > 0 && H.ncols == (n > 0 ? n - 1 : 0), "tridiag: householder must be block_size x (n - 1)");
	FH_CHECK(n < (1L << 30), "tridiag: matrix too large");
	if (n <= 1)
		return;
	hipStream_t s = ctx().stream;
	const idx_t nbr = (n + TF_TR - 1) / TF_TR, ncb = (n + TF_TC - 1) / TF_TC;
	Scratch vb((size_t) (4 * n) * sizeof(T) + 256), cb((size_t) (1 + ncb + nbr) * (size_t) n * sizeof(double)), stb(sizeof(TdState)),
		cntb((size_t) (ncb + 1) * sizeof(xwg_u64));
	TdArgs<T> a;
	a.force_mem = g_l2_force_mem.load();
	a.A = A.p;
	a.rs = A.rs;
	a.cs = A.cs;
	a.n = (int) n;
	a.y = vb.as<T>();
	a.w = a.y + n;
	a.taus = a.w + 2 * n;
	a.ysum = cb.as<double>();
	a.rpart = a.ysum + n;
	a.cpart = a.rpart + (size_t) ncb * (size_t) n;
	a.flags = cntb.as<xwg_u64>();
	a.st = stb.as<TdState>();
	FH_HIP(hipMemsetAsync(vb.p, 0, (size_t) (4 * n) * sizeof(T), s));
	FH_HIP(hipMemsetAsync(stb.p, 0, sizeof(TdState), s));
	FH_HIP(hipMemsetAsync(cntb.p, 0, (size_t) (ncb + 1) * sizeof(xwg_u64), s));
	for (idx_t k = 0; k < n; ++k) {
		a.k = (int) k;
		// block 0: the step; blocks 1 ..: the sums of the previous pass (k > 0), one per index block of TF_TC entries
		const unsigned nsb = k > 0 ? (unsigned) ((n - k - 1 + TF_TC - 1) / TF_TC) : 0u;
		hipLaunchKernelGGL(td_step_kernel<T>, dim3(1 + nsb), dim3(LV2_NT), 0, s, a);
		const idx_t r = n - k - 2;
		if (r > 0) {
			const idx_t rb = (r + TF_TR - 1) / TF_TR;
			if (k > 0)
				hipLaunchKernelGGL((td_fused_kernel<T, true>), dim3((unsigned) (rb * (rb + 1))), dim3(TF_NT), 0, s, a);
			else
				hipLaunchKernelGGL((td_fused_kernel<T, false>), dim3((unsigned) (rb * (rb + 1))), dim3(TF_NT), 0, s, a);
		}
	}
	FH_HIP(hipGetLastError());
	// block Householder factors of A.submatrix(1, 0, n - 1, n - 1) (:516-533)
	qr_t_blocks_from_taus<T>(A.sub(1, 0, n - 1, n - 1), H, n - 1, a.taus);
	FH_HIP(hipStreamSynchronize(s)); // the scratch vectors above are released on return
}
template void tridiag_dev<double>(MatV<double>, MatV<double>);
template void tridiag_dev<float>(MatV<float>, MatV<float>);

// ------------------------------------------------------------------------------------------------
// Bidiagonalization -- faer/src/linalg/svd/bidiag.rs:47-255.
// The reference's unblocked level-2 algorithm: per column k (i) column k and row k receive the rest of the previous
// step's rank-2 update (:80-98), (ii) the left reflector of column k (:99-102), (iii) ONE pass over A22 that applies
// A22 -= up y2 + z2 vp and forms y2 = u^H A22 (bidiag_fused_op, :257-301), (iv) y2, row k and its norm (:156-164),
// (v) z2 = A22 A12^H (:165-172), (vi) the right reflector of the normalised row and the correction of z2 (:176-213).
// Four launches per column, no host synchronisation in the loop:
//   bd_pre_kernel(k)   block 0: (vi)'s correction of z for step k-1, then (i) and (ii); blocks 1 ..: the sums of the row pass of step k-1
//   bd_col_kernel(k)   256 x 32 tiles of A22, lanes along the rows, 32 loads in flight per thread: (iii) written back and the tile's
//                      share of y2 = u^H A22
//   bd_mid_kernel(k)   block 0: (iv), a copy of the normalised row for (v), then the reflector part of (vi); blocks 1 ..: the sums of
//                      the column pass
//   bd_row_kernel(k)   128 x 128 tiles of A22 (read only): the tile's share of (v)
// The shares of the tiles are added in a fixed order (bd_sum_block) and handed to block 0 inside the launch (xwg.h).  Rounds 2-5: one
// wavefront per column / one workgroup per 16 rows with complete sums (302 ms at N = 4096); tiles with sums as launches of their own:
// 272; pre / mid with their rows and columns in registers: 230; the sums as helper blocks: 210.
// Algorithmic bytes: A22 read + written once and read once more per column, sum_k 3 (m-k-1)(n-k-1) sizeof(T).
// ------------------------------------------------------------------------------------------------
struct BdState {
	double tl_inv;			  // left reflector of the current step
	double tr_inv, beta, hinv, b, norm; // right reflector of the current step (consumed by the next bd_pre_kernel)
	int hinv_inf, pad;
};
template <typename T> struct BdArgs {
	T *A;
	idx_t rs, cs;
	int m, n, size, k, force_mem;
	T *y, *z, *vrow, *taul, *taur;
	double *ysum, *zsum;   // u^H A22 and A22 v of the two passes, complete (fixed-order sums of the shares below)
	double *ypart, *zpart; // shares of the tiles: ypart[row block * n + j], zpart[column block * m + i]
	xwg_u64 *yflag, *zflag; // per helper block of bd_mid_kernel / bd_pre_kernel: the launch whose sums are complete
	int nh;		       // helper blocks of this launch (0: the sums were prepared otherwise)
	BdState *st;
};

constexpr int BC_TR = 256, BC_TC = 32, BC_NT = 256; // tiles of bd_col_kernel
constexpr int BR_TR = 128, BR_TC = 128, BR_NT = 256; // tiles of bd_row_kernel
// Helper block h of a single-workgroup launch: out[off + e] = the sum of `np` shares part[p * stride + off + e], e in [1024 h, 1024 h + 1024)
// and < len, added in the order of p; stored write-through and flagged, because the reader is block 0 of the SAME launch (xwg.h; the
// tridiagonalization's td_sum_block has the reasoning).  All 1024 threads of the calling workgroup.
static __device__ __forceinline__ void bd_sum_block(const double *part, int np, size_t stride, int off, int len, double *out, int h)
{
	const int e = h * LV2_NT + (int) threadIdx.x;
	if (e >= len)
		return;
	const double *src = part + off + e;
	xwg_store(out + off + e, lv2_sum_shares(src, np, stride));
}
// which = 0: z sums of row pass k - 1 for bd_pre_kernel(k) (rows k .., column blocks of BR_TC); 1: y sums of column pass k for
// bd_mid_kernel(k) (columns k + 1 .., row blocks of BC_TR)
template <typename T> static __device__ __forceinline__ void bd_helper(const BdArgs<T> &a, int which, int h)
{
	if (which == 0)
		bd_sum_block(a.zpart, (a.n - a.k + BR_TC - 1) / BR_TC, (size_t) a.m, a.k, a.m - a.k, a.zsum, h);
	else
		bd_sum_block(a.ypart, (a.m - a.k - 1 + BC_TR - 1) / BC_TR, (size_t) a.n, a.k + 1, a.n - a.k - 1, a.ysum, h);
}
template <typename T> static __device__ __forceinline__ void bd_helper_block(const BdArgs<T> &a, int which)
{
	bd_helper<T>(a, which, (int) blockIdx.x - 1);
	lv2_helper_done((which == 0 ? a.zflag : a.yflag) + (blockIdx.x - 1), (xwg_u64) (a.k + 1));
}
// block 0: the sums are complete (or it adds the shares itself if the helpers' flags do not come)
template <typename T> static __device__ __forceinline__ void bd_wait_sums(const BdArgs<T> &a, int which)
{
	__shared__ int s_flag;
	if (a.nh <= 0)
		return;
	if (!xwg_wait_all(which == 0 ? a.zflag : a.yflag, a.nh, (xwg_u64) (a.k + 1), &s_flag)) {
		for (int h = 0; h < a.nh; ++h)
			bd_helper<T>(a, which, h);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
	}
}

template <typename T> static __device__ __forceinline__ void bd_pre_body(const BdArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	const int tid = threadIdx.x, k = a.k, m = a.m, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T nacc[3] = {0, 0, 0};
	if (k > 0) {
		// ---- z of step k-1 (:186-213): zsum = A22 A12^H of that step, u = its left reflector (column k-1), A22_a = column k
		const T beta = (T) a.st->beta, hinv = (T) a.st->hinv, b = (T) a.st->b, tr_inv = (T) a.st->tr_inv;
		const bool inf = a.st->hinv_inf != 0;
		auto fix = [&](T zs, T a22a, T u) -> T {
			T w;
			if (!inf) {
				w = zs - a22a * beta;
				w = w * hinv;
				w = w - u * b;
			} else {
				w = a22a - u * b;
			}
			return w * tr_inv;
		};
		bd_wait_sums<T>(a, 0);
		const T up0 = at(k, k - 1), y1 = a.y[k];
		const T z1 = fix((T) xwg_load(a.zsum + k), at(k, k), up0);
		__syncthreads(); // everyone has read a_kk
		// ---- (i): the rest of the previous rank-2 update on column k, row k and a_kk (:80-98)
		if (tid == 0) {
			a.z[k] = z1;
			at(k, k) -= up0 * y1 + z1;
		}
		for (int i = k + 1 + tid; i < m; i += LV2_NT) {
			const T u = at(i, k - 1), old = at(i, k);
			const T zf = fix((T) xwg_load(a.zsum + i), old, u);
			a.z[i] = zf;
			const T v = old - (u * y1 + zf);
			at(i, k) = v;
			LV2_NORM_ACC(nacc, v, sml, big);
		}
		for (int j = k + 1 + tid; j < n; j += LV2_NT)
			at(k, j) -= up0 * a.y[j] + z1 * at(k - 1, j);
	} else {
		for (int i = 1 + tid; i < m; i += LV2_NT) {
			const T v = at(i, 0);
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	}
	// ---- (ii) left reflector of column k (:99-102)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = at(k, k), hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	__syncthreads(); // everyone has read the old head
	if (!negligible)
		for (int i = k + 1 + tid; i < m; i += LV2_NT)
			at(i, k) *= hinv;
	if (tid == 0) {
		at(k, k) = head;
		a.taul[k] = tau;
		a.st->tl_inv = (double) ((T) 1 / tau);
	}
}

template <typename T> static __device__ __forceinline__ void bd_mid_body(const BdArgs<T> &a);

// bd_pre_body with every entry it touches in registers (at most LV2_E per thread and direction): all loads -- the strided ones of rows k - 1
// and k among them -- are issued at the start, every entry is stored once.  Same arithmetic, expression by expression.
template <typename T> static __device__ __forceinline__ void bd_pre_body_reg(const BdArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	const int tid = threadIdx.x, k = a.k, m = a.m, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const bool upd = k > 0;
	T cu[LV2_E], cold[LV2_E], czs[LV2_E], rk[LV2_E], rkm[LV2_E], ry[LV2_E];
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + 1 + tid + e * LV2_NT, ic = i < m ? i : m - 1;
		cold[e] = at(ic, k);
		cu[e] = upd ? at(ic, k - 1) : (T) 0;
		czs[e] = (T) 0;
		const int j = k + 1 + tid + e * LV2_NT, jc = j < n ? j : n - 1;
		rk[e] = upd ? at(k, jc) : (T) 0;
		rkm[e] = upd ? at(k - 1, jc) : (T) 0;
		ry[e] = upd ? a.y[jc] : (T) 0;
	}
	T akk = at(k, k);
	T nacc[3] = {0, 0, 0};
	if (upd) {
		const T beta = (T) a.st->beta, hinv = (T) a.st->hinv, b = (T) a.st->b, tr_inv = (T) a.st->tr_inv;
		const bool inf = a.st->hinv_inf != 0;
		auto fix = [&](T zs, T a22a, T u) -> T {
			T w;
			if (!inf) {
				w = zs - a22a * beta;
				w = w * hinv;
				w = w - u * b;
			} else {
				w = a22a - u * b;
			}
			return w * tr_inv;
		};
		const T up0 = at(k, k - 1), y1 = a.y[k];
		bd_wait_sums<T>(a, 0); // (the loads above are in flight while the helper blocks finish the sums)
#pragma unroll
		for (int e = 0; e < LV2_E; ++e) {
			const int i = k + 1 + tid + e * LV2_NT;
			czs[e] = (T) xwg_load(a.zsum + (i < m ? i : m - 1));
		}
		const T z1 = fix((T) xwg_load(a.zsum + k), akk, up0);
		akk -= up0 * y1 + z1;
		if (tid == 0)
			a.z[k] = z1; // (a_kk itself is stored once, below, as the reflector's beta: nobody may see an intermediate value)
#pragma unroll
		for (int e = 0; e < LV2_E; ++e) {
			const int i = k + 1 + tid + e * LV2_NT;
			if (i < m) {
				const T zf = fix(czs[e], cold[e], cu[e]);
				a.z[i] = zf;
				cold[e] = cold[e] - (cu[e] * y1 + zf);
			}
			const int j = k + 1 + tid + e * LV2_NT;
			if (j < n)
				at(k, j) = rk[e] - (up0 * ry[e] + z1 * rkm[e]);
		}
	}
#pragma unroll
	for (int e = 0; e < LV2_E; ++e)
		if (k + 1 + tid + e * LV2_NT < m) {
			const T v = cold[e];
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	// ---- (ii) left reflector of column k (:99-102)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = akk, hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + 1 + tid + e * LV2_NT;
		if (i < m && (upd || !negligible))
			at(i, k) = negligible ? cold[e] : cold[e] * hinv;
	}
	if (tid == 0) {
		at(k, k) = head;
		a.taul[k] = tau;
		a.st->tl_inv = (double) ((T) 1 / tau);
	}
}

template <typename T> __global__ __launch_bounds__(LV2_NT) void bd_pre_kernel(const BdArgs<T> a)
{
	if (blockIdx.x > 0) {
		bd_helper_block<T>(a, 0);
		return;
	}
	if (a.m - a.k - 1 <= LV2_E * LV2_NT && a.n - a.k - 1 <= LV2_E * LV2_NT && !a.force_mem)
		bd_pre_body_reg<T>(a);
	else
		bd_pre_body<T>(a);
}

// bd_mid_body with row k in registers: ONE strided read and one strided write of the row instead of three each.
template <typename T> static __device__ __forceinline__ void bd_mid_body_reg(const BdArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	__shared__ T s_bc[1];
	const int tid = threadIdx.x, k = a.k, n = a.n;
	auto row = [&](int j) -> T & { return a.A[(idx_t) k * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const T tl_inv = (T) a.st->tl_inv;
	T v[LV2_E], yv[LV2_E];
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int j = k + 1 + tid + e * LV2_NT, jc = j < n ? j : n - 1;
		v[e] = row(jc);
	}
	bd_wait_sums<T>(a, 1); // (the strided loads of the row are in flight meanwhile)
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int j = k + 1 + tid + e * LV2_NT;
		yv[e] = (T) xwg_load(a.ysum + (j < n ? j : n - 1));
	}
	// ---- (iv) y2 = (y2 + A12) / tau_l, A12 -= y2, norm of A12 (:156-164)
	T nacc[3] = {0, 0, 0};
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int j = k + 1 + tid + e * LV2_NT;
		if (j < n) {
			yv[e] = (yv[e] + v[e]) * tl_inv;
			a.y[j] = yv[e];
			v[e] = v[e] - yv[e];
			LV2_NORM_ACC(nacc, v[e], sml, big);
		}
	}
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T norm = norm_from3<T>(s_red);
	const T norm_inv = (T) 1 / norm;
	T tacc[3] = {0, 0, 0};
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int j = k + 1 + tid + e * LV2_NT;
		if (j < n) {
			if (norm != (T) 0)
				v[e] *= norm_inv;
			a.vrow[j] = v[e]; // (v) multiplies by the normalised row as it is BEFORE the right reflector touches it
			if (j >= k + 2) {
				LV2_NORM_ACC(tacc, v[e], sml, big);
			}
		}
	}
	if (k + 1 >= a.size) {
#pragma unroll
		for (int e = 0; e < LV2_E; ++e)
			if (k + 1 + tid + e * LV2_NT < n)
				row(k + 1 + tid + e * LV2_NT) = v[e];
		return;
	}
	if (tid == 0)
		s_bc[0] = v[0]; // the head of the row (j = k + 1)
	// ---- (vi) right reflector of the normalised row (:176-185) and b (:186-193)
	double tad[3] = {(double) tacc[0], (double) tacc[1], (double) tacc[2]};
	block_sum<LV2_NT, 3>(tad, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = s_bc[0], hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	double d[1] = {0.0};
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int j = k + 1 + tid + e * LV2_NT;
		if (j < n && j >= k + 2) {
			if (!negligible)
				v[e] *= hinv;
			row(j) = v[e];
			d[0] += (double) yv[e] * (double) v[e];
		}
	}
	block_sum<LV2_NT, 1>(d, s_part, s_red);
	if (tid == 0) {
		const T b = yv[0] + (T) s_red[0];
		row(k + 1) = head * norm; // beta, rescaled (:183-184)
		a.taur[k] = tau;
		a.st->tr_inv = (double) ((T) 1 / tau);
		a.st->beta = (double) head;
		a.st->hinv = (double) hinv;
		a.st->hinv_inf = negligible ? 1 : 0;
		a.st->b = (double) b;
		a.st->norm = (double) norm;
	}
}

template <typename T> __global__ __launch_bounds__(LV2_NT) void bd_mid_kernel(const BdArgs<T> a)
{
	if (blockIdx.x > 0) {
		bd_helper_block<T>(a, 1);
		return;
	}
	if (a.n - a.k - 1 <= LV2_E * LV2_NT && !a.force_mem)
		bd_mid_body_reg<T>(a);
	else
		bd_mid_body<T>(a);
}

// (iii): tile of BC_TR rows x BC_TC columns of A22 = A[k+1.., k+1..]; wavefront w owns 8 columns, a lane four rows of each (32 loads in
// flight per thread): A22 -= up y2 + z2 vp written back, and the tile's share of y2 = u^H A22 -> ypart[row block][column].
template <typename T, bool upd> __global__ __launch_bounds__(BC_NT) void bd_col_kernel(const BdArgs<T> a)
{
	constexpr int CW = BC_TC / (BC_NT / 64), RH = BC_TR / 64; // 8 columns per wavefront, 4 rows per lane
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k;
	const int base = k + 1, rr = a.m - base, cc = a.n - base;
	const int ncb = (cc + BC_TC - 1) / BC_TC;
	const int I = blockIdx.x / ncb, J = blockIdx.x - I * ncb;
	const int i0 = I * BC_TR, j0 = J * BC_TC + CW * wv;
	T *A22 = a.A + (idx_t) base * a.rs + (idx_t) base * a.cs;
	const T *ucol = a.A + (idx_t) base * a.rs + (idx_t) k * a.cs;		    // u_i (the left reflector, rows base..)
	const T *upcol = a.A + (idx_t) base * a.rs + (idx_t) (upd ? k - 1 : 0) * a.cs; // up_i
	const T *vprow = a.A + (idx_t) (upd ? k - 1 : 0) * a.rs + (idx_t) base * a.cs; // vp_j (row k - 1)
	int gi[RH];
	bool vr[RH];
	T ui[RH], upi[RH], zi[RH];
#pragma unroll
	for (int h = 0; h < RH; ++h) {
		gi[h] = i0 + lane + 64 * h;
		vr[h] = gi[h] < rr;
		gi[h] = min(gi[h], rr - 1);
		const idx_t o = (idx_t) gi[h] * a.rs;
		ui[h] = ucol[o];
		upi[h] = upd ? upcol[o] : (T) 0;
		zi[h] = upd ? a.z[base + gi[h]] : (T) 0;
	}
	T yjl = (T) 0, vpjl = (T) 0; // column values of the wavefront's columns, one per lane
	if (upd) {
		const int gj = min(j0 + (lane & (CW - 1)), cc - 1);
		yjl = a.y[base + gj];
		vpjl = vprow[(idx_t) gj * a.cs];
	}
	T v[RH][CW];
#pragma unroll
	for (int c = 0; c < CW; ++c)
#pragma unroll
		for (int h = 0; h < RH; ++h)
			v[h][c] = A22[(idx_t) gi[h] * a.rs + (idx_t) min(j0 + c, cc - 1) * a.cs];
#pragma unroll
	for (int c = 0; c < CW; ++c) {
		const int gj = j0 + c;
		const T yj = lv2_lane(yjl, c), vpj = lv2_lane(vpjl, c);
		double cs_ = 0.0;
#pragma unroll
		for (int h = 0; h < RH; ++h) {
			const bool in = vr[h] && gj < cc;
			T tv = v[h][c];
			if (upd) {
				tv = fh_fma(-upi[h], yj, tv); // A22 -= up y2 (:292)
				tv = fh_fma(-zi[h], vpj, tv); // A22 -= z2 vp (:293)
				if (in)
					A22[(idx_t) gi[h] * a.rs + (idx_t) gj * a.cs] = tv;
			}
			cs_ += in ? (double) ui[h] * (double) tv : 0.0; // y2 = u^H A22 (:294-300)
		}
		const double sv = lv2_wave_sum(cs_);
		if (lane == 0 && gj < cc)
			a.ypart[(size_t) I * a.n + base + gj] = sv;
	}
}

template <typename T> static __device__ __forceinline__ void bd_mid_body(const BdArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	const int tid = threadIdx.x, k = a.k, n = a.n;
	auto row = [&](int j) -> T & { return a.A[(idx_t) k * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const T tl_inv = (T) a.st->tl_inv;
	// ---- (iv) y2 = (y2 + A12) / tau_l, A12 -= y2, norm of A12 (:156-164)
	T nacc[3] = {0, 0, 0};
	bd_wait_sums<T>(a, 1);
	for (int j = k + 1 + tid; j < n; j += LV2_NT) {
		const T yv = ((T) xwg_load(a.ysum + j) + row(j)) * tl_inv;
		a.y[j] = yv;
		const T v = row(j) - yv;
		row(j) = v;
		LV2_NORM_ACC(nacc, v, sml, big);
	}
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T norm = norm_from3<T>(s_red);
	const T norm_inv = (T) 1 / norm;
	T tacc[3] = {0, 0, 0};
	for (int j = k + 1 + tid; j < n; j += LV2_NT) {
		T v = row(j);
		if (norm != (T) 0) {
			v *= norm_inv;
			row(j) = v;
		}
		a.vrow[j] = v; // (v) multiplies by the normalised row as it is BEFORE the right reflector touches it
		if (j >= k + 2) {
			LV2_NORM_ACC(tacc, v, sml, big);
		}
	}
	if (k + 1 >= a.size)
		return;
	// ---- (vi) right reflector of the normalised row (:176-185) and b (:186-193)
	double tad[3] = {(double) tacc[0], (double) tacc[1], (double) tacc[2]};
	block_sum<LV2_NT, 3>(tad, s_part, s_red); // (its barriers publish the row written above)
	const T tail_norm = norm_from3<T>(s_red);
	T head = row(k + 1), hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	__syncthreads(); // everyone has read the old head
	double d[1] = {0.0};
	for (int j = k + 2 + tid; j < n; j += LV2_NT) {
		T v = row(j);
		if (!negligible) {
			v *= hinv;
			row(j) = v;
		}
		d[0] += (double) a.y[j] * (double) v;
	}
	block_sum<LV2_NT, 1>(d, s_part, s_red);
	if (tid == 0) {
		const T b = a.y[k + 1] + (T) s_red[0];
		row(k + 1) = head * norm; // beta, rescaled (:183-184)
		a.taur[k] = tau;
		a.st->tr_inv = (double) ((T) 1 / tau);
		a.st->beta = (double) head;
		a.st->hinv = (double) hinv;
		a.st->hinv_inf = negligible ? 1 : 0;
		a.st->b = (double) b;
		a.st->norm = (double) norm;
	}
}

// (v): z2 = A22 A12^H with the normalised row (vrow), read only: tile of BR_TR rows x BR_TC columns; wavefront w owns 32 columns, a lane two
// rows of each (64 loads in two batches); the tile's share of the row sums -> zpart[column block][row].
template <typename T> __global__ __launch_bounds__(BR_NT) void bd_row_kernel(const BdArgs<T> a)
{
	constexpr int CW = BR_TC / (BR_NT / 64); // 32 columns per wavefront
	__shared__ double s_row[BR_NT / 64][BR_TR];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k;
	const int base = k + 1, rr = a.m - base, cc = a.n - base;
	const int ncb = (cc + BR_TC - 1) / BR_TC;
	const int I = blockIdx.x / ncb, J = blockIdx.x - I * ncb;
	const int i0 = I * BR_TR, j0 = J * BR_TC + CW * wv;
	const T *A22 = a.A + (idx_t) base * a.rs + (idx_t) base * a.cs;
	int gi[2];
#pragma unroll
	for (int h = 0; h < 2; ++h)
		gi[h] = min(i0 + lane + 64 * h, rr - 1);
	double racc[2] = {0.0, 0.0};
#pragma unroll
	for (int cb = 0; cb < CW; cb += 16) {
		const int gjl = min(j0 + cb + (lane & 15), cc - 1);
		const T xl = (j0 + cb + (lane & 15) < cc) ? a.vrow[base + gjl] : (T) 0; // (columns past the end contribute nothing)
		T v[2][16];
#pragma unroll
		for (int c = 0; c < 16; ++c)
#pragma unroll
			for (int h = 0; h < 2; ++h)
				v[h][c] = A22[(idx_t) gi[h] * a.rs + (idx_t) min(j0 + cb + c, cc - 1) * a.cs];
#pragma unroll
		for (int c = 0; c < 16; ++c) {
			const T xj = lv2_lane(xl, c);
#pragma unroll
			for (int h = 0; h < 2; ++h)
				racc[h] += (double) v[h][c] * (double) xj;
		}
	}
	s_row[wv][lane] = racc[0];
	s_row[wv][lane + 64] = racc[1];
	__syncthreads();
	if (tid < BR_TR && i0 + tid < rr)
		a.zpart[(size_t) J * a.m + base + i0 + tid] = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
}

// A: m x n; Hl: bl x min(m, n), Hr: br x (min(m, n) - 1)
template <typename T> void bidiag_dev(MatV<T> A, MatV<T> Hl, MatV<T> Hr)
{
	const idx_t m = A.nrows, n = A.ncols;
	// (m < n runs like the reference does -- svd/bidiag.rs loops over min(m, n) columns and leaves the last row of a wide
	// matrix normalised, without its right reflector; its SVD only ever passes tall matrices)
	const idx_t size = m < n ? m : n;
	FH_CHECK(Hl.ncols == size && Hr.ncols == (size > 0 ? size - 1 : 0), "bidiag: householder factors must have n and n - 1 columns");
	FH_CHECK((Hl.nrows > 0 || size == 0) && (Hr.nrows > 0 || size <= 1), "bidiag: householder factors need at least one row");
	FH_CHECK(m < (1L << 30) && n < (1L << 30), "bidiag: matrix too large");
	if (size == 0)
		return;
	hipStream_t s = ctx().stream;
	const idx_t nrb = (m + BC_TR - 1) / BC_TR, ncb = (n + BR_TC - 1) / BR_TC;
	const idx_t nhy = (n + LV2_NT - 1) / LV2_NT, nhz = (m + LV2_NT - 1) / LV2_NT; // helper blocks of bd_mid_kernel / bd_pre_kernel at most
	Scratch vb((size_t) (4 * n + m) * sizeof(T) + 256), stb(sizeof(BdState)), pb((size_t) (nrb * n + ncb * m + n + m) * sizeof(double)),
		fb((size_t) (nhy + nhz) * sizeof(xwg_u64));
	BdArgs<T> a;
	a.force_mem = g_l2_force_mem.load();
	a.A = A.p;
	a.rs = A.rs;
	a.cs = A.cs;
	a.m = (int) m;
	a.n = (int) n;
	a.size = (int) size;
	a.y = vb.as<T>();
	a.vrow = a.y + n;
	a.z = a.vrow + n;
	a.taul = a.z + m;
	a.taur = a.taul + n;
	a.ypart = pb.as<double>();
	a.zpart = a.ypart + (size_t) nrb * (size_t) n;
	a.ysum = a.zpart + (size_t) ncb * (size_t) m;
	a.zsum = a.ysum + n;
	a.yflag = fb.as<xwg_u64>();
	a.zflag = a.yflag + nhy;
	a.st = stb.as<BdState>();
	FH_HIP(hipMemsetAsync(vb.p, 0, (size_t) (4 * n + m) * sizeof(T), s));
	FH_HIP(hipMemsetAsync(a.ysum, 0, (size_t) (n + m) * sizeof(double), s));
	FH_HIP(hipMemsetAsync(fb.p, 0, (size_t) (nhy + nhz) * sizeof(xwg_u64), s));
	FH_HIP(hipMemsetAsync(stb.p, 0, sizeof(BdState), s));
	bool have_z = false; // a row pass has left shares for the next bd_pre_kernel
	for (idx_t k = 0; k < size; ++k) {
		a.k = (int) k;
		const idx_t rr = m - k - 1, cc = n - k - 1;
		// block 0: the step; blocks 1 ..: the sums of the previous row pass (1024 entries each)
		a.nh = have_z ? (int) ((m - k + LV2_NT - 1) / LV2_NT) : 0;
		hipLaunchKernelGGL(bd_pre_kernel<T>, dim3((unsigned) (1 + a.nh)), dim3(LV2_NT), 0, s, a);
		have_z = false;
		if (cc > 0) {
			a.nh = 0;
			if (rr > 0) {
				const unsigned rb = (unsigned) ((rr + BC_TR - 1) / BC_TR), cb = (unsigned) ((cc + BC_TC - 1) / BC_TC);
				if (k > 0)
					hipLaunchKernelGGL((bd_col_kernel<T, true>), dim3(rb * cb), dim3(BC_NT), 0, s, a);
				else
					hipLaunchKernelGGL((bd_col_kernel<T, false>), dim3(rb * cb), dim3(BC_NT), 0, s, a);
				a.nh = (int) ((cc + LV2_NT - 1) / LV2_NT);
			} else {
				FH_HIP(hipMemsetAsync(a.ysum + k + 1, 0, (size_t) cc * sizeof(double), s)); // (no row below: y2 = 0)
			}
			hipLaunchKernelGGL(bd_mid_kernel<T>, dim3((unsigned) (1 + a.nh)), dim3(LV2_NT), 0, s, a);
			if (k + 1 < size && rr > 0) {
				const unsigned rb = (unsigned) ((rr + BR_TR - 1) / BR_TR), cb = (unsigned) ((cc + BR_TC - 1) / BR_TC);
				hipLaunchKernelGGL(bd_row_kernel<T>, dim3(rb * cb), dim3(BR_NT), 0, s, a);
				have_z = true;
			}
		}
	}
	FH_HIP(hipGetLastError());
	// block Householder factors (:216-254): the left ones are in the QR layout, the right ones in its transpose
	qr_t_blocks_from_taus<T>(A, Hl, size, a.taul);
	if (size > 1)
		qr_t_blocks_from_taus<T>(A.sub(0, 1, size - 1, n - 1).t(), Hr, size - 1, a.taur);
	FH_HIP(hipStreamSynchronize(s)); // the scratch vectors above are released on return
}
template void bidiag_dev<double>(MatV<double>, MatV<double>, MatV<double>);
template void bidiag_dev<float>(MatV<float>, MatV<float>, MatV<float>);

// ------------------------------------------------------------------------------------------------
// Hessenberg reduction -- faer/src/linalg/evd/hessenberg.rs:230-408 (hessenberg_rearranged_unblocked; SURVEY.md section
// 8f item 4).  The reference switches to a blocked variant (hessenberg_gqvdg_blocked, :568-736) for n >= 256: the same
// reflectors of the same columns in another order of operations; this path runs the level-2 variant at every size (its
// passes are HBM streams here, not cache-blocked loops) and agrees with either up to rounding.
// Per column k: (i) row k, column k and a_kk receive the rest of the previous two-sided update (:266-281), (ii) the
// reflector of column k below the subdiagonal, head = 1 while the step runs (:294-305), (iii) ONE pass over A22 applying
// A22 -= u2 y2 + z2 u2^H and forming x^H A22 and A22 x (hessenberg_fused_op, :149-193), (iv) y2, z2 (:342-357), (v) the
// reflector from the right on row k and the rows above it (:358-378).  Three launches per column (round 6):
//   hs_pre_kernel(k)    block 0: (iv) of step k-1, restores its beta, (i), (ii); blocks 1 ..: w of step k-1 from the shares of its
//                       top-rows pass, and the application dwp = w / tau it leaves pending
//   hs_fused_kernel(k)  128 x 64 tiles of A22: the update written back and the tile's shares of BOTH x^H A22 and A22 x (same x)
//   hs_top_kernel(k)    128 x 64 tiles of the rows 0 .. k: the pending application of step k-1 written back, the shares of this
//                       step's w; extra blocks add the shares of hs_fused_kernel -> ysum, zsum
// Traffic per column: A22 and the k+1 rows above read and written ONCE (the reference's count -- and rounds 2-5 -- read A22 twice and the
// rows above twice).  N = 4096 fp64: 257.6 ms (round 5) -> 219 (one fused pass over A22) -> 165 (deferred application on the rows above).
// ------------------------------------------------------------------------------------------------
struct HsState {
	double tau_inv, beta;
};
template <typename T> struct HsArgs {
	T *A;
	idx_t rs, cs;
	int n, k, force_mem;
	T *y, *z, *ysum, *zsum, *taus;
	double *ypart, *zpart; // shares of the tiles of the fused pass: ypart[row block * n + j], zpart[column block * n + i]
	double *wpart;	       // shares of the tiles of the top-rows pass: wpart[column block * n + i]
	T *dwp;		       // per row i <= k - 1: w_i / tau of step k - 1, the right-side application that is still pending (0: none)
	HsState *st;
};

template <typename T> static __device__ __forceinline__ void hs_pre_body(const HsArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	const int tid = threadIdx.x, k = a.k, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T nacc[3] = {0, 0, 0};
	if (k > 0) {
		// ---- (iv) of step k-1 (:342-357): x = [1; A[k+1.., k-1]] (its head is still 1 in memory), zsum = A22 x, ysum = x^H A22
		const T tau_inv = (T) a.st->tau_inv;
		double d[1] = {0.0};
		for (int i = k + tid; i < n; i += LV2_NT)
			d[0] += (double) at(i, k - 1) * (double) a.zsum[i];
		block_sum<LV2_NT, 1>(d, s_part, s_red);
		const T b = ((T) s_red[0] * (T) 0.5) * tau_inv;
		const T x0 = at(k, k - 1); // == 1
		const T y1 = (a.ysum[k] - b * x0) * tau_inv, z1 = (a.zsum[k] - b * x0) * tau_inv;
		__syncthreads(); // everyone has read the head of the previous reflector
		// ---- (i) (:266-281) fused with the rest of (iv)
		if (tid == 0) {
			at(k, k - 1) = (T) a.st->beta; // (:379) the previous reflector's head goes back to beta
			a.y[k] = y1;
			a.z[k] = z1;
			at(k, k) -= y1 + z1;
		}
		for (int i = k + 1 + tid; i < n; i += LV2_NT) {
			const T u = at(i, k - 1);
			const T yi = (a.ysum[i] - b * u) * tau_inv, zi = (a.zsum[i] - b * u) * tau_inv;
			a.y[i] = yi;
			a.z[i] = zi;
			at(k, i) -= yi + z1 * u;	    // row k: A12 -= y2 + z1 u2^H
			const T v = at(i, k) - (u * y1 + zi); // column k: A21 -= u2 y1 + z2
			at(i, k) = v;
			if (i >= k + 2) {
				LV2_NORM_ACC(nacc, v, sml, big);
			}
		}
	} else {
		for (int i = 2 + tid; i < n; i += LV2_NT) {
			const T v = at(i, 0);
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	}
	if (k + 1 >= n)
		return;
	// ---- (ii) reflector of column k below the subdiagonal (:294-305)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = at(k + 1, k), hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
	__syncthreads(); // everyone has read the old head
	if (!negligible)
		for (int i = k + 2 + tid; i < n; i += LV2_NT)
			at(i, k) *= hinv;
	if (tid == 0) {
		at(k + 1, k) = (T) 1; // head of x while the step runs; beta comes back in the next hs_pre_kernel
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		a.st->beta = (double) head;
	}
}

// hs_pre_body with column k - 1, column k, row k and the two products in registers (n - k <= LV2_E LV2_NT): one round trip to memory, every
// entry stored once.  Same arithmetic, expression by expression.
template <typename T> static __device__ __forceinline__ void hs_pre_body_reg(const HsArgs<T> &a)
{
	__shared__ double s_part[(LV2_NT / 64) * 3], s_red[3];
	__shared__ T s_bc[1];
	const int tid = threadIdx.x, k = a.k, n = a.n;
	auto at = [&](int i, int j) -> T & { return a.A[(idx_t) i * a.rs + (idx_t) j * a.cs]; };
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const bool upd = k > 0;
	// rows / columns i = k + tid + e LV2_NT
	T u[LV2_E], ck[LV2_E], rk[LV2_E], ys[LV2_E], zs[LV2_E];
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + tid + e * LV2_NT, ic = i < n ? i : n - 1;
		ck[e] = at(ic, k);
		u[e] = upd ? at(ic, k - 1) : (T) 0;
		rk[e] = upd ? at(k, ic) : (T) 0;
		ys[e] = upd ? a.ysum[ic] : (T) 0;
		zs[e] = upd ? a.zsum[ic] : (T) 0;
	}
	T nacc[3] = {0, 0, 0};
	if (upd) {
		// ---- (iv) of step k-1 (:342-357)
		const T tau_inv = (T) a.st->tau_inv, x0 = at(k, k - 1), ysk = a.ysum[k], zsk = a.zsum[k], beta = (T) a.st->beta;
		double d[1] = {0.0};
#pragma unroll
		for (int e = 0; e < LV2_E; ++e)
			if (k + tid + e * LV2_NT < n)
				d[0] += (double) u[e] * (double) zs[e];
		block_sum<LV2_NT, 1>(d, s_part, s_red);
		const T b = ((T) s_red[0] * (T) 0.5) * tau_inv;
		const T y1 = (ysk - b * x0) * tau_inv, z1 = (zsk - b * x0) * tau_inv;
		// ---- (i) (:266-281) fused with the rest of (iv)
#pragma unroll
		for (int e = 0; e < LV2_E; ++e) {
			const int i = k + tid + e * LV2_NT;
			if (i < n && i >= k + 1) {
				const T yi = (ys[e] - b * u[e]) * tau_inv, zi = (zs[e] - b * u[e]) * tau_inv;
				a.y[i] = yi;
				a.z[i] = zi;
				at(k, i) = rk[e] - (yi + z1 * u[e]);   // row k: A12 -= y2 + z1 u2^H
				ck[e] = ck[e] - (u[e] * y1 + zi);       // column k: A21 -= u2 y1 + z2
			}
		}
		if (tid == 0) {
			at(k, k - 1) = beta; // (:379) the previous reflector's head goes back to beta
			a.y[k] = y1;
			a.z[k] = z1;
			at(k, k) = ck[0] - (y1 + z1);
		}
	}
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + tid + e * LV2_NT;
		if (i < n && i >= k + 2) {
			const T v = ck[e];
			LV2_NORM_ACC(nacc, v, sml, big);
		}
	}
	if (k + 1 >= n)
		return;
	if (tid == 1)
		s_bc[0] = ck[0]; // row k + 1: the head of the column
	// ---- (ii) reflector of column k below the subdiagonal (:294-305)
	double accd[3] = {(double) nacc[0], (double) nacc[1], (double) nacc[2]};
	block_sum<LV2_NT, 3>(accd, s_part, s_red);
	const T tail_norm = norm_from3<T>(s_red);
	T head = s_bc[0], hinv;
	bool negligible;
	const T tau = lv2_householder<T>(head, tail_norm, hinv, negligible);
#pragma unroll
	for (int e = 0; e < LV2_E; ++e) {
		const int i = k + tid + e * LV2_NT;
		if (i < n && i >= k + 2 && (upd || !negligible))
			at(i, k) = negligible ? ck[e] : ck[e] * hinv;
	}
	if (tid == 0) {
		at(k + 1, k) = (T) 1; // head of x while the step runs; beta comes back in the next hs_pre_kernel
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		a.st->beta = (double) head;
	}
}

template <typename T> __global__ __launch_bounds__(LV2_NT) void hs_pre_kernel(const HsArgs<T> a)
{
	if (blockIdx.x > 0) {
		// helper block: rows 1024 (blockIdx.x - 1) ..: w of step k - 1 = the shares of its top-rows pass in a fixed order, then the
		// pending application dwp = w / tau_{k-1} for hs_top_kernel(k).  Independent of block 0 (which overwrites st->tau_inv: taken from taus)
		const int k = a.k, i = ((int) blockIdx.x - 1) * LV2_NT + (int) threadIdx.x;
		if (i >= k)
			return;
		const int np = (a.n - (k - 1) + TF_TC - 1) / TF_TC;
		a.dwp[i] = (T) lv2_sum_shares(a.wpart + i, np, (size_t) a.n) * ((T) 1 / a.taus[k - 1]);
		return;
	}
	if (a.n - a.k <= LV2_E * LV2_NT && !a.force_mem)
		hs_pre_body_reg<T>(a);
	else
		hs_pre_body<T>(a);
}

// Round 6: both products of a step use the SAME x, so ONE pass over A22 = A[k+1.., k+1..] applies the two-sided update of the previous step
// and forms the tile's shares of l_out = x^H A22 (column sums) and r_out = A22 x (row sums): 128 x 64 tiles as in the tridiagonalization
// (lane = two rows, wavefront = 16 columns, 32 loads in flight per thread); the shares are added in a fixed order by extra blocks of hs_top_kernel.
// The rows above (0 .. k, which receive the reflector from the right once their sums are complete) stay with hs_rowpass_kernel.
template <typename T, bool upd> __global__ __launch_bounds__(TF_NT) void hs_fused_kernel(const HsArgs<T> a)
{
	constexpr int CW = TF_TC / (TF_NT / 64); // 16 columns per wavefront
	__shared__ double s_row[TF_NT / 64][TF_TR];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k;
	const int base = k + 1, r = a.n - base;
	const int ncb = (r + TF_TC - 1) / TF_TC;
	const int I = blockIdx.x / ncb, J = blockIdx.x - I * ncb;
	const int i0 = I * TF_TR, j0 = J * TF_TC + CW * wv;
	T *A22 = a.A + (idx_t) base * a.rs + (idx_t) base * a.cs;
	const T *xcol = a.A + (idx_t) base * a.rs + (idx_t) k * a.cs;		    // x (head = 1 in memory)
	const T *ucol = a.A + (idx_t) base * a.rs + (idx_t) (upd ? k - 1 : 0) * a.cs; // u2: the previous reflector's tail
	int gi[2];
	bool vr[2];
	T xi[2], ui[2], zi[2];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		gi[h] = i0 + lane + 64 * h;
		vr[h] = gi[h] < r;
		gi[h] = min(gi[h], r - 1);
		const idx_t o = (idx_t) gi[h] * a.rs;
		xi[h] = xcol[o];
		ui[h] = upd ? ucol[o] : (T) 0;
		zi[h] = upd ? a.z[base + gi[h]] : (T) 0;
	}
	T xjl, yjl = (T) 0, ujl = (T) 0;
	{
		const int gj = min(j0 + (lane & (CW - 1)), r - 1);
		xjl = xcol[(idx_t) gj * a.rs];
		if (upd) {
			yjl = a.y[base + gj];
			ujl = ucol[(idx_t) gj * a.rs];
		}
	}
	T v[2][CW];
#pragma unroll
	for (int c = 0; c < CW; ++c)
#pragma unroll
		for (int h = 0; h < 2; ++h)
			v[h][c] = A22[(idx_t) gi[h] * a.rs + (idx_t) min(j0 + c, r - 1) * a.cs];
	double racc[2] = {0.0, 0.0};
#pragma unroll
	for (int c = 0; c < CW; ++c) {
		const int gj = j0 + c;
		const T xj = lv2_lane(xjl, c), yj = lv2_lane(yjl, c), uj = lv2_lane(ujl, c);
		double cs_ = 0.0;
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const bool in = vr[h] && gj < r;
			T tv = v[h][c];
			if (upd) {
				tv = fh_fma(-ui[h], yj, tv); // A22 -= u2 y2      (:160-167)
				tv = fh_fma(-zi[h], uj, tv); // A22 -= z2 u2^H    (:168-175)
				if (in)
					A22[(idx_t) gi[h] * a.rs + (idx_t) gj * a.cs] = tv;
			}
			cs_ += in ? (double) xi[h] * (double) tv : 0.0;	 // l_out = x^H A22 (:184-191)
			racc[h] += in ? (double) tv * (double) xj : 0.0; // r_out = A22 x   (:176-183)
		}
		const double sv = lv2_wave_sum(cs_);
		if (lane == 0 && gj < r)
			a.ypart[(size_t) I * a.n + base + gj] = sv;
	}
	s_row[wv][lane] = racc[0];
	s_row[wv][lane + 64] = racc[1];
	__syncthreads();
	if (tid < TF_TR && i0 + tid < r)
		a.zpart[(size_t) J * a.n + base + i0 + tid] = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
}

// Rows 0 .. k (hs_fused_kernel has the rows below): their sums with x are the w of the right-side application (:358-378), A[0..k, k+1..] -=
// (w / tau) x^H.  Rounds 2-5 gave 16 rows to a workgroup that summed them and then applied the reflector (every row read twice per step).
// Round 6: the application is DEFERRED by one step and rides on the next step's pass -- tile (rows 0 .. k) x (columns k .. n-1): entries
// first receive the pending application of step k - 1 (dwp_i x_{k-1,j}; column k only that: it is final afterwards), are written back, and
// contribute to the new sums with x_k; the shares of the tiles are added by helper blocks of the next hs_pre_kernel, which also turn them
// into the next dwp.  One read and one write per entry and step; a last call behind the loop (k = n - 1) applies what is still pending.
// The blocks behind the tiles add the shares of hs_fused_kernel in a fixed order -> ysum, zsum (one launch less per column).
template <typename T> __global__ __launch_bounds__(TF_NT) void hs_top_kernel(const HsArgs<T> a)
{
	constexpr int CW = TF_TC / (TF_NT / 64); // 16 columns per wavefront
	__shared__ double s_row[TF_NT / 64][TF_TR];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k, n = a.n;
	const int nrows = k + 1, ncols = n - k; // rows 0 .. k, columns k .. n - 1
	const int ncb = (ncols + TF_TC - 1) / TF_TC, nrb = (nrows + TF_TR - 1) / TF_TR;
	if ((int) blockIdx.x >= nrb * ncb) {
		const int r = n - (k + 1);
		const int e = ((int) blockIdx.x - nrb * ncb) * TF_NT + tid;
		if (e >= 2 * r)
			return;
		const bool isz = e >= r;
		const int np = isz ? (r + TF_TC - 1) / TF_TC : (r + TF_TR - 1) / TF_TR;
		const double *src = (isz ? a.zpart : a.ypart) + (k + 1) + (isz ? e - r : e);
		(isz ? a.zsum : a.ysum)[(k + 1) + (isz ? e - r : e)] = (T) lv2_sum_shares(src, np, (size_t) n);
		return;
	}
	const bool upd = k > 0;
	const int I = blockIdx.x / ncb, J = blockIdx.x - I * ncb;
	const int i0 = I * TF_TR, j0 = k + J * TF_TC + CW * wv; // (absolute column)
	int gi[2];
	bool vr[2];
	T dwi[2];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		gi[h] = i0 + lane + 64 * h;
		vr[h] = gi[h] < nrows;
		gi[h] = min(gi[h], nrows - 1);
		dwi[h] = upd ? a.dwp[gi[h]] : (T) 0;
	}
	T xpl, xnl; // per lane: the pending reflector x_{k-1} and the new one x_k at this wavefront's columns
	{
		const int gj = min(j0 + (lane & (CW - 1)), n - 1);
		xpl = !upd ? (T) 0 : (gj == k ? (T) 1 : a.A[(idx_t) gj * a.rs + (idx_t) (k - 1) * a.cs]);
		xnl = gj >= k + 1 ? a.A[(idx_t) gj * a.rs + (idx_t) k * a.cs] : (T) 0; // (head = 1 in memory while the step runs)
	}
	T v[2][CW];
#pragma unroll
	for (int c = 0; c < CW; ++c)
#pragma unroll
		for (int h = 0; h < 2; ++h)
			v[h][c] = a.A[(idx_t) gi[h] * a.rs + (idx_t) min(j0 + c, n - 1) * a.cs];
	double racc[2] = {0.0, 0.0};
#pragma unroll
	for (int c = 0; c < CW; ++c) {
		const int gj = j0 + c;
		const T xp = lv2_lane(xpl, c), xn = lv2_lane(xnl, c);
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const bool in = vr[h] && gj < n;
			T tv = v[h][c];
			if (upd) {
				tv = tv - dwi[h] * xp;
				if (in)
					a.A[(idx_t) gi[h] * a.rs + (idx_t) gj * a.cs] = tv;
			}
			racc[h] += in ? (double) tv * (double) xn : 0.0;
		}
	}
	s_row[wv][lane] = racc[0];
	s_row[wv][lane + 64] = racc[1];
	__syncthreads();
	if (tid < TF_TR && i0 + tid < nrows)
		a.wpart[(size_t) J * n + i0 + tid] = ((s_row[0][tid] + s_row[1][tid]) + s_row[2][tid]) + s_row[3][tid];
}

// A: n x n, H: block_size x (n - 1)
template <typename T> void hessenberg_dev(MatV<T> A, MatV<T> H)
{
	const idx_t n = A.nrows;
	FH_CHECK(A.ncols == n, "hessenberg: the matrix must be square");
	FH_CHECK(H.ncols == (n > 0 ? n - 1 : 0), "hessenberg: householder must be block_size x (n - 1)");
	FH_CHECK(n < (1L << 30), "hessenberg: matrix too large");
	if (n <= 1)
		return;
	FH_CHECK(H.nrows > 0, "hessenberg: householder needs at least one row");
	hipStream_t s = ctx().stream;
	const idx_t nrb = (n + TF_TR - 1) / TF_TR, ncb = (n + TF_TC - 1) / TF_TC;
	Scratch vb((size_t) (6 * n) * sizeof(T) + 256), stb(sizeof(HsState)), pb((size_t) (nrb + 2 * ncb) * (size_t) n * sizeof(double));
	HsArgs<T> a;
	a.force_mem = g_l2_force_mem.load();
	a.ypart = pb.as<double>();
	a.zpart = a.ypart + (size_t) nrb * (size_t) n;
	a.wpart = a.zpart + (size_t) ncb * (size_t) n;
	a.A = A.p;
	a.rs = A.rs;
	a.cs = A.cs;
	a.n = (int) n;
	a.y = vb.as<T>();
	a.z = a.y + n;
	a.ysum = a.z + n;
	a.zsum = a.ysum + n;
	a.taus = a.zsum + n;
	a.dwp = a.taus + n;
	a.st = stb.as<HsState>();
	FH_HIP(hipMemsetAsync(vb.p, 0, (size_t) (6 * n) * sizeof(T), s));
	FH_HIP(hipMemsetAsync(stb.p, 0, sizeof(HsState), s));
	auto launch_top = [&](idx_t k) {
		const idx_t r = n - k - 1;
		const unsigned tiles = (unsigned) (((k + 1 + TF_TR - 1) / TF_TR) * ((n - k + TF_TC - 1) / TF_TC));
		hipLaunchKernelGGL(hs_top_kernel<T>, dim3(tiles + (unsigned) ((2 * r + TF_NT - 1) / TF_NT)), dim3(TF_NT), 0, s, a);
	};
	for (idx_t k = 0; k < n; ++k) {
		a.k = (int) k;
		// block 0: the step; blocks 1 ..: w of step k - 1 and the pending application it leaves (1024 rows each)
		hipLaunchKernelGGL(hs_pre_kernel<T>, dim3((unsigned) (1 + (k + LV2_NT - 1) / LV2_NT)), dim3(LV2_NT), 0, s, a);
		const idx_t r = n - k - 1;
		if (r > 0) {
			const unsigned rb = (unsigned) ((r + TF_TR - 1) / TF_TR), cb = (unsigned) ((r + TF_TC - 1) / TF_TC);
			if (k > 0)
				hipLaunchKernelGGL((hs_fused_kernel<T, true>), dim3(rb * cb), dim3(TF_NT), 0, s, a);
			else
				hipLaunchKernelGGL((hs_fused_kernel<T, false>), dim3(rb * cb), dim3(TF_NT), 0, s, a);
			launch_top(k);
		}
	}
	// the application of the last step (k = n - 2) is still pending on column n - 1
	a.k = (int) (n - 1);
	launch_top(n - 1);
	FH_HIP(hipGetLastError());
	qr_t_blocks_from_taus<T>(A.sub(1, 0, n - 1, n - 1), H, n - 1, a.taus); // (:382-406)
	FH_HIP(hipStreamSynchronize(s)); // the scratch vectors above are released on return
}
template void hessenberg_dev<double>(MatV<double>, MatV<double>);
template void hessenberg_dev<float>(MatV<float>, MatV<float>);

} // namespace fh
