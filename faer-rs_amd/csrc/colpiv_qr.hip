// QR with column pivoting -- faer/src/linalg/qr/col_pivoting/factor.rs:107-395.
// A level-2, HBM-bound algorithm like the reference's: per step the remaining column of largest (down-dated) norm is
// swapped in, its reflector is made, and the trailing rank-1 update is DELAYED by one step and fused with the dot
// products of the next one (update_mat_and_dot_simd, :7-105) unless the best down-dated norm fell below
// sqrt(eps) x the best norm at the last recomputation (:178-203: apply at once, recompute all norms).
// Five small launches per step, no host synchronisation inside the loop; one workgroup per column in the passes
// over the trailing matrix (lanes along the rows), the pivot search over the n norms by one workgroup.
#include <limits>
#include <vector>

#include "common.h"
#include "perm.h"
#include "reduce.h"
#include "xwg.h"

namespace fh {

struct CpState {
	double best_threshold, scale_fwd, scale_bwd;
	double l, tau_inv;
	int delayed, best_col, n_trans, flush; // flush: this step applies the pending update at once and recomputes the norms (:178-203)
	int timeout, pad;		       // the flush blocks of a step did not report (GPU shared with other work)
};

template <typename T> struct CpArgs {
	T *A;
	idx_t rs, cs;
	int m, n, size, k, delayed_ok;
	T *norm, *dot, *taus;
	int *perm;
	xwg_u64 *flags; // per flush block: the step it has finished (cp_step_kernel)
	CpState *st;
};

// norm_l2 (reductions/norm_l2.rs) of rows r0.. of column j by one workgroup of 256 threads
template <typename T> static __device__ T cp_col_norm(const CpArgs<T> &a, int r0, int j, double *s_part, double *s_red)
{
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T acc[3] = {0, 0, 0};
	for (int i = r0 + threadIdx.x; i < a.m; i += 256) {
		const T x = a.A[(idx_t) i * a.rs + (idx_t) j * a.cs];
		acc[0] += (x * sml) * (x * sml);
		acc[1] += x * x;
		acc[2] += (x * big) * (x * big);
	}
	double accd[3] = {(double) acc[0], (double) acc[1], (double) acc[2]};
	block_sum<256, 3>(accd, s_part, s_red);
	const T r = norm_from3<T>(s_red);
	__syncthreads();
	return r;
}

template <typename T> __global__ __launch_bounds__(256) void cp_norms_kernel(const CpArgs<T> a)
{
	__shared__ double s_part[4 * 3], s_red[3];
	const int j = blockIdx.x;
	const T v = cp_col_norm<T>(a, 0, j, s_part, s_red);
	if (threadIdx.x == 0)
		a.norm[j] = v;
}

// first maximum (strict '>') of norm[lo .. n)
template <typename T, bool COH = false> static __device__ void cp_argmax(const T *norm, int lo, int n, T &best, int &col, double *s_v, int *s_c)
{
	T bv = (T) 0;
	int bc = lo;
	for (int j = lo + threadIdx.x; j < n; j += blockDim.x) {
		const T v = COH ? xwg_load(norm + j) : norm[j];
		if (v > bv) { // ascending j per thread: the first maximum of the thread's subsequence
			bv = v;
			bc = j;
		}
	}
	double v = (double) bv;
	int cidx = bc;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const double ov = __shfl_xor(v, off, 64);
		const int oc = __shfl_xor(cidx, off, 64);
		if (ov > v || (ov == v && ov > 0.0 && oc < cidx)) {
			v = ov;
			cidx = oc;
		}
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0) {
		s_v[wave] = v;
		s_c[wave] = cidx;
	}
	__syncthreads();
	v = s_v[0];
	cidx = s_c[0];
	for (int w = 1; w < (int) blockDim.x / 64; ++w)
		if (s_v[w] > v || (s_v[w] == v && s_v[w] > 0.0 && s_c[w] < cidx)) {
			v = s_v[w];
			cidx = s_c[w];
		}
	__syncthreads();
	best = (T) v;
	col = v > 0.0 ? cidx : lo;
}

// factor.rs:142-160: scale by the reciprocal of the largest column norm
template <typename T> __global__ __launch_bounds__(1024) void cp_init_kernel(const CpArgs<T> a)
{
	__shared__ double s_v[16];
	__shared__ int s_c[16];
	T best;
	int col;
	cp_argmax<T>(a.norm, 0, a.n, best, col, s_v, s_c);
	const T scale_bwd = (T) 1 / best;
	for (int j = threadIdx.x; j < a.n; j += 1024) {
		a.norm[j] = a.norm[j] * scale_bwd;
		a.dot[j] = (T) 0;
		a.perm[j] = j;
	}
	if (threadIdx.x == 0) {
		a.st->scale_fwd = (double) best;
		a.st->scale_bwd = (double) scale_bwd;
		a.st->best_threshold = (double) ((best * scale_bwd) * (T) sqrt((double) Lim<T>::eps));
		a.st->n_trans = 0;
	}
}

// A *= scale (all of it with `upper` == 0, the upper triangle with the diagonal otherwise)
template <typename T> __global__ void cp_scale_kernel(const CpArgs<T> a, int upper)
{
	const T sc = (T) (upper ? a.st->scale_fwd : a.st->scale_bwd);
	const idx_t total = (idx_t) a.m * a.n;
	for (idx_t e = (idx_t) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (idx_t) gridDim.x * blockDim.x) {
		const idx_t i = e % a.m, j = e / a.m;
		if (!upper || i <= j)
			a.A[i * a.rs + j * a.cs] *= sc;
	}
}

// factor.rs:204-252: column swap, the pending update of column k, its reflector (householder.rs:59-107)
// COH: the columns and norms may have been rewritten by the flush blocks of the SAME launch (cp_step_kernel): every read of them
// passes the caches
template <typename T, bool COH = false> static __device__ __forceinline__ void cp_house_body(const CpArgs<T> &a, const int bc, const int delayed)
{
	auto ld = [&](const T *q) -> T { return COH ? xwg_load(q) : *q; };

	__shared__ double s_part[16 * 3], s_red[3];
	const int tid = threadIdx.x, k = a.k;
	if (bc != k) {
		for (int i = tid; i < a.m; i += 1024) {
			T *p = a.A + (idx_t) i * a.rs + (idx_t) k * a.cs, *q = a.A + (idx_t) i * a.rs + (idx_t) bc * a.cs;
			const T x = ld(p), y = ld(q);
			*p = y;
			*q = x;
		}
		if (tid == 0) {
			const int tp = a.perm[k];
			a.perm[k] = a.perm[bc];
			a.perm[bc] = tp;
			const T td = a.dot[k], tn = ld(a.norm + k);
			a.dot[k] = a.dot[bc];
			a.dot[bc] = td;
			a.norm[k] = ld(a.norm + bc);
			a.norm[bc] = tn;
			a.st->n_trans += 1;
		}
	}
	__syncthreads();
	const T l = delayed ? a.A[(idx_t) k * a.rs + (idx_t) (k - 1) * a.cs] : (T) 0;
	const T r = a.dot[k];
	__syncthreads();
	// pending update of column k and the scaled sums of its tail in one pass
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T acc[3] = {0, 0, 0};
	for (int i = k + 1 + tid; i < a.m; i += 1024) {
		T *p = a.A + (idx_t) i * a.rs + (idx_t) k * a.cs;
		T x = ld(p);
		if (delayed) {
			x += r * a.A[(idx_t) i * a.rs + (idx_t) (k - 1) * a.cs];
			*p = x;
		}
		acc[0] += (x * sml) * (x * sml);
		acc[1] += x * x;
		acc[2] += (x * big) * (x * big);
	}
	double accd[3] = {(double) acc[0], (double) acc[1], (double) acc[2]};
	{ // 16 waves
		const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const double sv = wave_sum(accd[c]);
			if (lane == 0)
				s_part[wave * 3 + c] = sv;
		}
		__syncthreads();
		if (tid < 3) {
			double t = 0.0;
			for (int w = 0; w < 16; ++w)
				t += s_part[w * 3 + tid];
			s_red[tid] = t;
		}
		__syncthreads();
	}
	const T tail_norm = norm_from3<T>(s_red);
	T *hp = a.A + (idx_t) k * a.rs + (idx_t) k * a.cs;
	T head = ld(hp);
	if (delayed)
		head += l * r;
	T head_norm = fabs(head);
	if (head_norm < Lim<T>::minpos) {
		head = (T) 0;
		head_norm = (T) 0;
	}
	T tau, hinv = (T) 0;
	bool scale_tail = false;
	if (tail_norm < Lim<T>::minpos) {
		tau = std::numeric_limits<T>::infinity();
	} else {
		const T norm = (T) hypot((double) head_norm, (double) tail_norm);
		const T sign = head_norm != (T) 0 ? head * ((T) 1 / head_norm) : (T) 1;
		const T signed_norm = sign * norm;
		hinv = (T) 1 / (head + signed_norm);
		head = -signed_norm;
		const T tn = tail_norm * fabs(hinv);
		tau = (T) 0.5 * ((T) 1 + tn * tn);
		scale_tail = true;
	}
	__syncthreads();
	if (scale_tail)
		for (int i = k + 1 + tid; i < a.m; i += 1024)
		{
				T *pp = a.A + (idx_t) i * a.rs + (idx_t) k * a.cs;
				*pp = ld(pp) * hinv;
			}
	if (tid == 0) {
		*hp = head;
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		a.st->l = (double) l;
	}
	if (k + 1 == a.size && delayed) // factor.rs:253-262
		for (int j = k + 1 + tid; j < a.n; j += 1024)
			a.A[(idx_t) k * a.rs + (idx_t) j * a.cs] += l * a.dot[j];
}

// cp_house_body with the two swapped columns and column k - 1 in registers (m <= 4 x 1024 rows): one round trip to memory after the pivot
// is known instead of three (swap, pending update, scaling), every entry stored once.  Same arithmetic, expression by expression.
template <typename T, bool COH> static __device__ __forceinline__ void cp_house_body_reg(const CpArgs<T> &a, const int bc, const int delayed)
{
	auto ld = [&](const T *q) -> T { return COH ? xwg_load(q) : *q; };
	constexpr int E = 4;
	__shared__ double s_part[16 * 3], s_red[3];
	__shared__ T s_head;
	const int tid = threadIdx.x, k = a.k, m = a.m;
	const bool sw = bc != k;
	T ck[E], cb[E], c1[E];
#pragma unroll
	for (int e = 0; e < E; ++e) {
		const int i = tid + e * 1024, ic = i < m ? i : m - 1;
		ck[e] = ld(a.A + (idx_t) ic * a.rs + (idx_t) k * a.cs);
		cb[e] = sw ? ld(a.A + (idx_t) ic * a.rs + (idx_t) bc * a.cs) : ck[e];
		c1[e] = delayed ? a.A[(idx_t) ic * a.rs + (idx_t) (k - 1) * a.cs] : (T) 0;
	}
	const T l = delayed ? a.A[(idx_t) k * a.rs + (idx_t) (k - 1) * a.cs] : (T) 0;
	const T r = a.dot[sw ? bc : k];
	T tn_k = (T) 0, tn_b = (T) 0;
	if (tid == 0 && sw) {
		tn_k = ld(a.norm + k);
		tn_b = ld(a.norm + bc);
	}
	__syncthreads(); // every read of dot / norm / perm is done
	if (tid == 0 && sw) {
		const int tp = a.perm[k];
		a.perm[k] = a.perm[bc];
		a.perm[bc] = tp;
		const T td = a.dot[k];
		a.dot[k] = r;
		a.dot[bc] = td;
		a.norm[k] = tn_b;
		a.norm[bc] = tn_k;
		a.st->n_trans += 1;
	}
	// pending update of column k and the scaled sums of its tail
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	T acc[3] = {0, 0, 0};
#pragma unroll
	for (int e = 0; e < E; ++e) {
		const int i = tid + e * 1024;
		if (i < m && i >= k + 1) {
			T x = cb[e];
			if (delayed)
				x += r * c1[e];
			cb[e] = x;
			acc[0] += (x * sml) * (x * sml);
			acc[1] += x * x;
			acc[2] += (x * big) * (x * big);
		}
		if (i == k)
			s_head = cb[e];
	}
	double accd[3] = {(double) acc[0], (double) acc[1], (double) acc[2]};
	{ // 16 waves
		const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const double sv = wave_sum(accd[c]);
			if (lane == 0)
				s_part[wave * 3 + c] = sv;
		}
		__syncthreads();
		if (tid < 3) {
			double t = 0.0;
			for (int w = 0; w < 16; ++w)
				t += s_part[w * 3 + tid];
			s_red[tid] = t;
		}
		__syncthreads();
	}
	const T tail_norm = norm_from3<T>(s_red);
	T head = s_head;
	if (delayed)
		head += l * r;
	T head_norm = fabs(head);
	if (head_norm < Lim<T>::minpos) {
		head = (T) 0;
		head_norm = (T) 0;
	}
	T tau, hinv = (T) 0;
	bool scale_tail = false;
	if (tail_norm < Lim<T>::minpos) {
		tau = std::numeric_limits<T>::infinity();
	} else {
		const T norm = (T) hypot((double) head_norm, (double) tail_norm);
		const T sign = head_norm != (T) 0 ? head * ((T) 1 / head_norm) : (T) 1;
		const T signed_norm = sign * norm;
		hinv = (T) 1 / (head + signed_norm);
		head = -signed_norm;
		const T tn = tail_norm * fabs(hinv);
		tau = (T) 0.5 * ((T) 1 + tn * tn);
		scale_tail = true;
	}
#pragma unroll
	for (int e = 0; e < E; ++e) {
		const int i = tid + e * 1024;
		if (i < m) {
			if (sw)
				a.A[(idx_t) i * a.rs + (idx_t) bc * a.cs] = ck[e];
			T *pk = a.A + (idx_t) i * a.rs + (idx_t) k * a.cs;
			if (i > k) {
				if (sw || delayed || scale_tail)
					*pk = scale_tail ? cb[e] * hinv : cb[e];
			} else if (i == k) {
				*pk = head;
			} else if (sw) {
				*pk = cb[e];
			}
		}
	}
	if (tid == 0) {
		a.taus[k] = tau;
		a.st->tau_inv = (double) ((T) 1 / tau);
		a.st->l = (double) l;
	}
	if (k + 1 == a.size && delayed) // factor.rs:253-262
		for (int j = k + 1 + tid; j < a.n; j += 1024)
			a.A[(idx_t) k * a.rs + (idx_t) j * a.cs] += l * a.dot[j];
}
template <typename T, bool COH> static __device__ __forceinline__ void cp_house(const CpArgs<T> &a, const int bc, const int delayed)
{
	if (a.m <= 4 * 1024)
		cp_house_body_reg<T, COH>(a, bc, delayed);
	else
		cp_house_body<T, COH>(a, bc, delayed);
}

// Round 6: ONE launch per step.  Block 0 (factor.rs:163-177): the best remaining column by the down-dated norms and the decision "delayed
// update or recompute", published to the other blocks of the launch (one flag word: 2 (k + 1) + recompute).  Common case: the column swap
// and the reflector follow in block 0 and the other blocks leave as soon as they see the flag.  Recompute (:178-203, k > 0): blocks 1 ..
// apply the pending update to the trailing columns, A11 += A10[:, k-1] dot[k:], and recompute their norms (a column per block and turn; the
// first 256 threads work, with the strides and the sum order of the 256-thread kernel this replaces), write-through, then raise their flag;
// block 0 waits for the flags, picks the pivot from the fresh norms and makes the reflector -- reading what the other blocks wrote past its
// caches.  Rounds 1-5: select, flush, select2, house = four launches, two of them returning at once on almost every step (3-5 us each).
constexpr int CP_NFL = 15; // helper blocks
template <typename T> __global__ __launch_bounds__(1024) void cp_step_kernel(const CpArgs<T> a)
{
	__shared__ double s_v[16];
	__shared__ int s_c[16];
	__shared__ double s_part[16 * 3], s_red[3];
	__shared__ int s_flag;
	const int tid = threadIdx.x, k = a.k;
	xwg_u64 *dflag = a.flags + CP_NFL;
	if (blockIdx.x > 0) {
		// ---- helper block: wait for block 0's decision
		if (tid == 0) {
			int dec = -1;
			for (int spin = 0; spin < (1 << 21); ++spin) {
				const xwg_u64 v = __hip_atomic_load(dflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if ((v >> 1) == (xwg_u64) (k + 1)) {
					dec = (int) (v & 1);
					break;
				}
				__builtin_amdgcn_s_sleep(2);
			}
			s_flag = dec;
		}
		__syncthreads();
		if (s_flag != 1)
			return; // (no recomputation -- or block 0 never spoke: it reports the time-out itself)
		const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
		for (int j = k + (int) blockIdx.x - 1; j < a.n; j += (int) gridDim.x - 1) {
			const T d = a.dot[j];
			T acc[3] = {0, 0, 0};
			if (tid < 256)
				for (int i = k + tid; i < a.m; i += 256) {
					T *p = a.A + (idx_t) i * a.rs + (idx_t) j * a.cs;
					const T x = fh_fma(a.A[(idx_t) i * a.rs + (idx_t) (k - 1) * a.cs], d, *p);
					xwg_store(p, x);
					acc[0] += (x * sml) * (x * sml);
					acc[1] += x * x;
					acc[2] += (x * big) * (x * big);
				}
			const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				const double sv = wave_sum((double) acc[c]);
				if (lane == 0)
					s_part[wave * 3 + c] = sv;
			}
			__syncthreads();
			if (tid < 3)
				s_red[tid] = s_part[tid] + s_part[3 + tid] + s_part[6 + tid] + s_part[9 + tid]; // (the four working wavefronts, in their order)
			__syncthreads();
			if (tid == 0)
				xwg_store(a.norm + j, norm_from3<T>(s_red));
			__syncthreads();
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
		if (tid == 0)
			__hip_atomic_store(a.flags + (blockIdx.x - 1), (xwg_u64) (k + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return;
	}
	// ---- block 0
	T best;
	int col;
	cp_argmax<T>(a.norm, k, a.n, best, col, s_v, s_c);
	const int delayed = (a.delayed_ok && k > 0 && (double) best >= a.st->best_threshold) ? 1 : 0;
	const int flush = k > 0 && !delayed;
	__syncthreads(); // (everyone has read the threshold)
	if (tid == 0) {
		if (gridDim.x > 1)
			__hip_atomic_store(dflag, ((xwg_u64) (k + 1) << 1) | (xwg_u64) flush, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		a.st->delayed = delayed;
		a.st->best_col = col;
		a.st->flush = flush;
	}
	if (!flush) {
		cp_house<T, false>(a, col, delayed);
		return;
	}
	// (a time-out cannot be repaired here -- the columns are half rewritten by then --: it is reported through the status word)
	if (!xwg_wait_all(a.flags, (int) gridDim.x - 1, (xwg_u64) (k + 1), &s_flag)) {
		if (tid == 0)
			a.st->timeout = 1;
		return;
	}
	cp_argmax<T, true>(a.norm, k, a.n, best, col, s_v, s_c);
	if (tid == 0) {
		a.st->best_col = col;
		a.st->best_threshold = (double) (best * (T) sqrt((double) Lim<T>::eps));
	}
	cp_house<T, true>(a, col, 0);
}

// factor.rs:266-301 / update_mat_and_dot_simd (:60-98): one workgroup per trailing column
template <typename T> __global__ __launch_bounds__(256) void cp_update_kernel(const CpArgs<T> a)
{
	__shared__ double s_part[4], s_red[1];
	const int k = a.k, j = k + 1 + blockIdx.x, tid = threadIdx.x;
	const int delayed = a.st->delayed;
	const T b0 = a.dot[j];
	T acc = (T) 0;
	for (int i = k + 1 + tid; i < a.m; i += 256) {
		T *p = a.A + (idx_t) i * a.rs + (idx_t) j * a.cs;
		T dst = *p;
		if (delayed) {
			dst = fh_fma(a.A[(idx_t) i * a.rs + (idx_t) (k - 1) * a.cs], b0, dst);
			*p = dst;
		}
		acc = fh_fma(a.A[(idx_t) i * a.rs + (idx_t) k * a.cs], dst, acc);
	}
	double accd[1] = {(double) acc};
	block_sum<256, 1>(accd, s_part, s_red);
	if (tid == 0) {
		const T tau_inv = (T) a.st->tau_inv, l = (T) a.st->l;
		T *up = a.A + (idx_t) k * a.rs + (idx_t) j * a.cs;
		T u;
		if (delayed) {
			const T tmp = *up + l * b0;
			const T d0 = (tmp + (T) s_red[0]) * (-tau_inv);
			u = tmp + d0;
			a.dot[j] = d0;
		} else {
			const T d = -((*up + (T) s_red[0]) * tau_inv);
			u = *up + d;
			a.dot[j] = d;
		}
		*up = u;
		const T nj = a.norm[j];
		a.norm[j] = sqrt(nj * nj - u * u);
	}
}

// A: m x n, H: block_size x min(m, n); col_perm / col_perm_inv: HOST arrays of n entries.  Returns the transposition count.
template <typename T> long colpiv_qr_dev(MatV<T> A, MatV<T> H, idx_t *col_perm, idx_t *col_perm_inv)
{
	const idx_t m = A.nrows, n = A.ncols;
	const idx_t size = m < n ? m : n;
	FH_CHECK(H.nrows > 0 && H.ncols == size, "colpiv_qr: Q_coeff must be block_size x min(nrows, ncols)");
	FH_CHECK(m < (1L << 30) && n < (1L << 30), "colpiv_qr: matrix too large");
	for (idx_t j = 0; j < n; ++j)
		col_perm[j] = col_perm_inv[j] = j;
	if (size == 0)
		return 0;
	hipStream_t s = ctx().stream;
	Scratch nb((size_t) (2 * n + size) * sizeof(T) + 256), pb((size_t) n * sizeof(int) + 256), stb(sizeof(CpState)), flb((size_t) (CP_NFL + 1) * sizeof(xwg_u64));
	CpArgs<T> a;
	a.flags = flb.as<xwg_u64>();
	FH_HIP(hipMemsetAsync(flb.p, 0, (size_t) (CP_NFL + 1) * sizeof(xwg_u64), s));
	a.A = A.p;
	a.rs = A.rs;
	a.cs = A.cs;
	a.m = (int) m;
	a.n = (int) n;
	a.size = (int) size;
	a.k = 0;
	a.delayed_ok = A.rs == 1 ? 1 : 0; // the reference's SIMD path needs column-major storage (factor.rs:174-176)
	a.norm = nb.as<T>();
	a.dot = a.norm + n;
	a.taus = a.dot + n;
	a.perm = pb.as<int>();
	a.st = stb.as<CpState>();
	FH_HIP(hipMemsetAsync(stb.p, 0, sizeof(CpState), s));
	hipLaunchKernelGGL(cp_norms_kernel<T>, dim3((unsigned) n), dim3(256), 0, s, a);
	hipLaunchKernelGGL(cp_init_kernel<T>, dim3(1), dim3(1024), 0, s, a);
	hipLaunchKernelGGL(cp_scale_kernel<T>, dim3(1024), dim3(256), 0, s, a, 0);
	for (idx_t k = 0; k < size; ++k) {
		a.k = (int) k;
		hipLaunchKernelGGL(cp_step_kernel<T>, dim3((unsigned) (k > 0 ? 1 + (n - k < CP_NFL ? n - k : CP_NFL) : 1)), dim3(1024), 0, s, a);
		if (k + 1 < size)
			hipLaunchKernelGGL(cp_update_kernel<T>, dim3((unsigned) (n - k - 1)), dim3(256), 0, s, a);
	}
	hipLaunchKernelGGL(cp_scale_kernel<T>, dim3(1024), dim3(256), 0, s, a, 1);
	FH_HIP(hipGetLastError());
	qr_t_blocks_from_taus<T>(A, H, size, a.taus);
	std::vector<int> hp((size_t) n);
	CpState fin;
	FH_HIP(hipMemcpyAsync(hp.data(), a.perm, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, s));
	FH_HIP(hipMemcpyAsync(&fin, stb.p, sizeof(fin), hipMemcpyDeviceToHost, s));
	FH_HIP(hipStreamSynchronize(s));
	FH_CHECK(!fin.timeout, "colpiv_qr: the blocks that recompute the column norms did not report in time (GPU shared with other work)");
	for (idx_t j = 0; j < n; ++j) {
		FH_CHECK(hp[(size_t) j] >= 0 && hp[(size_t) j] < n, "colpiv_qr: corrupt permutation");
		col_perm[j] = hp[(size_t) j];
	}
	invert_perm(n, col_perm, col_perm_inv);
	return fin.n_trans;
}
template long colpiv_qr_dev<double>(MatV<double>, MatV<double>, idx_t *, idx_t *);
template long colpiv_qr_dev<float>(MatV<float>, MatV<float>, idx_t *, idx_t *);

} // namespace fh
