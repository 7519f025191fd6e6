// Bunch-Kaufman factorization P A P^T = L B L^T of a symmetric indefinite matrix (include/faer_hip.h section 2g;
// faer/src/linalg/cholesky/bunch_kaufman/{factor,solve,reconstruct,inverse}.rs).  Only the lower triangle of A is read or
// written.  Strategies Partial, PartialDiag, Rook and RookDiag (the leaf and the W-panel below) and Full (a level-2 algorithm of its
// own, described in front of its kernels).
//
//  * Leaf (lblt_leaf_kernel): one workgroup keeps a trailing block of at most 64 rows in LDS as a full symmetric image and runs the
//    unblocked algorithm on it (factor.rs:784-902), rook loop included.  Every wavefront takes the pivot decisions redundantly from the
//    same image, so a step costs barriers only around the swaps and the elimination.
//  * Panel for more than 64 remaining rows (factor.rs:491-699, the W-panel algorithm): the trailing matrix is updated lazily.  Per pivot
//    step a multi-workgroup column kernel forms one candidate column w = a(:, i) - A_l W_l[i, :]^T (symmetric gather from the lower
//    triangle) with one arg-max candidate per workgroup; the second column pass decides by itself (every workgroup combines the first
//    pass's candidates in the same fixed order) whether it has to run; a single-workgroup pivot kernel takes the final decision, swaps,
//    scales, writes the L column(s), subdiag and the pivot record, updates the trailing diagonal and finds the next diagonal arg-max.
//    Everything is predicated on device state: Partial / PartialDiag panels run without a host synchronisation, Rook / RookDiag read
//    one flag back per rook iteration.  After the panel: one StrictTriangularLower MFMA product A_r -= W A_l^T, the LU row-interchange
//    kernel on the columns left of the panel, and one read-back of the panel's length (63 or 64).
//  * Ties of every arg-max go to the lowest index (strict >, rows in ascending order), as in the reference.
#include "common.h"
#include "perm.h"

using namespace fh;

extern "C" int faer_hip_lblt_pivoting_supported(FaerPivotingStrategy pivoting)
{
	const int p = (int) pivoting;
	return p >= (int) FaerPivotingStrategy_Partial && p <= (int) FaerPivotingStrategy_Full;
}

namespace {

constexpr int LB_NB = 64;   // panel width, most rows of the leaf
constexpr int LB_LDP = 65;  // pitch of the leaf's LDS image (odd: rows and columns are both conflict free)
constexpr int LB_NT = 256;  // threads of the leaf and of a column workgroup
constexpr int LB_PT = 1024; // threads of the pivot workgroup
constexpr int LB_NOIDX = 0x7fffffff;

// device state of a factorization
enum { ST_K = 0, ST_DONE, ST_I0, ST_I1, ST_NEED2, ST_NOTHING, ST_AGAIN, ST_N2X2, ST_COUNT = 16 };

template <typename T> struct Cand {
	T v;
	int i;
};

template <typename T> static __device__ __forceinline__ T lb_alpha() { return ((T) 1 + sqrt((T) 17)) * (T) 0.125; }

// larger value wins, equal values: the lower index
template <typename T, typename I> static __device__ __forceinline__ void wave_argmax(T &v, I &i)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const T ov = __shfl_xor(v, off, 64);
		const I oi = __shfl_xor(i, off, 64);
		if (ov > v || (ov == v && oi < i)) {
			v = ov;
			i = oi;
		}
	}
}

// workgroup arg-max of NT threads; every thread returns with the result.  s_v / s_i: NT / 64 entries.
template <typename T, int NT, typename I> static __device__ __forceinline__ void block_argmax(T &v, I &i, T *s_v, I *s_i)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	wave_argmax(v, i);
	__syncthreads(); // s_v / s_i may still be read from the previous use
	if (lane == 0) {
		s_v[wave] = v;
		s_i[wave] = i;
	}
	__syncthreads();
	v = s_v[0];
	i = s_i[0];
#pragma unroll
	for (int w = 1; w < NT / 64; ++w) {
		const T ov = s_v[w];
		const I oi = s_i[w];
		if (ov > v || (ov == v && oi < i)) {
			v = ov;
			i = oi;
		}
	}
}

// ------------------------------------------------------------------------------------------------ leaf
template <typename T> static __device__ __forceinline__ void leaf_sym_swap(T *S, int m, int a, int b)
{
	const int tid = threadIdx.x;
	if (tid < m) { // rows a, b over all columns
		const T x = S[tid * LB_LDP + a];
		S[tid * LB_LDP + a] = S[tid * LB_LDP + b];
		S[tid * LB_LDP + b] = x;
	}
	__syncthreads();
	if (tid < m) { // columns a, b over all rows
		const T x = S[a * LB_LDP + tid];
		S[a * LB_LDP + tid] = S[b * LB_LDP + tid];
		S[b * LB_LDP + tid] = x;
	}
	__syncthreads();
}

// max |S[r][idx]| over r in [k, m), r != idx (column idx of the symmetric image); gamma < 0: no such row
template <typename T> static __device__ __forceinline__ void leaf_offdiag(const T *S, int k, int m, int idx, T &gamma, int &r)
{
	const int lane = threadIdx.x & 63;
	gamma = (lane >= k && lane < m && lane != idx) ? fabs(S[idx * LB_LDP + lane]) : (T) -1;
	r = lane;
	wave_argmax(gamma, r);
}

// 1 x 1 elimination step of the leaf's image: pivot S[k][k], rows k + 1 .. m - 1 (factor.rs:855-868)
template <typename T> static __device__ __forceinline__ void leaf_eliminate_1x1(T *S, int k, int m)
{
	const int tid = threadIdx.x;
	const T dinv = (T) 1 / S[k * LB_LDP + k];
	const int mm = m - k - 1;
	for (int e = tid; e < mm * mm; e += LB_NT) {
		const int i = k + 1 + e % mm, j = k + 1 + e / mm;
		if (i < j)
			continue;
		const T w = S[k * LB_LDP + j] * dinv;
		const T v = fh_fma(S[k * LB_LDP + i], -w, S[j * LB_LDP + i]);
		S[j * LB_LDP + i] = v;
		S[i * LB_LDP + j] = v;
	}
	__syncthreads();
	if (tid > k && tid < m)
		S[k * LB_LDP + tid] *= dinv;
}

// 2 x 2 elimination step of the leaf's image: pivot rows k, k + 1 (factor.rs:869-897); returns a10, which the caller stores in subdiag
template <typename T> static __device__ __forceinline__ T leaf_eliminate_2x2(T *S, int k, int m)
{
	const int tid = threadIdx.x;
	const T a00 = S[k * LB_LDP + k], a11 = S[(k + 1) * LB_LDP + k + 1], a10 = S[k * LB_LDP + k + 1];
	const T d10_inv = (T) 1 / fabs(a10);
	const T d00 = a00 * d10_inv, d11 = a11 * d10_inv;
	const T t = (T) 1 / (d00 * d11 - (T) 1);
	const T d10 = a10 * d10_inv;
	const T d = t * d10_inv;
	const int mm = m - k - 2;
	for (int e = tid; e < mm * mm; e += LB_NT) {
		const int i = k + 2 + e % mm, j = k + 2 + e / mm;
		if (i < j)
			continue;
		const T x0 = S[k * LB_LDP + j], x1 = S[(k + 1) * LB_LDP + j];
		const T w0 = (x0 * d11 - x1 * d10) * d;
		const T w1 = (x1 * d00 - x0 * d10) * d;
		T v = S[j * LB_LDP + i];
		v = fh_fma(S[k * LB_LDP + i], -w0, v);
		v = fh_fma(S[(k + 1) * LB_LDP + i], -w1, v);
		S[j * LB_LDP + i] = v;
		S[i * LB_LDP + j] = v;
	}
	__syncthreads();
	if (tid > k + 1 && tid < m) {
		const T x0 = S[k * LB_LDP + tid], x1 = S[(k + 1) * LB_LDP + tid];
		S[k * LB_LDP + tid] = (x0 * d11 - x1 * d10) * d;
		S[(k + 1) * LB_LDP + tid] = (x1 * d00 - x0 * d10) * d;
	}
	return a10;
}

// A: the trailing m x m block (m <= 64); sub: its part of subdiag; piv: m pivot rows relative to the block; st: device state
template <typename T>
__global__ __launch_bounds__(LB_NT) void lblt_leaf_kernel(T *A, idx_t rs, idx_t cs, int m, T *sub, idx_t ss, int *piv, int *st, int rook,
							   int diagonal)
{
	__shared__ T S[LB_NB * LB_LDP];
	__shared__ T s_sub[LB_NB];
	__shared__ int s_piv[LB_NB];
	const int tid = threadIdx.x, lane = tid & 63;
	const T alpha = lb_alpha<T>();
	for (int e = tid; e < m * m; e += LB_NT) {
		const int i = e % m, j = e / m;
		S[j * LB_LDP + i] = j <= i ? A[(idx_t) i * rs + (idx_t) j * cs] : A[(idx_t) j * rs + (idx_t) i * cs];
	}
	int n2 = 0;
	int k = 0;
	while (k < m) {
		__syncthreads();
		// ---- decision: every wavefront computes the same one from the same image
		int i0 = k, i1 = -1, npiv = 1;
		if (diagonal) {
			T v = (lane >= k && lane < m) ? fabs(S[lane * LB_LDP + lane]) : (T) -1;
			i0 = lane;
			wave_argmax(v, i0);
		}
		T gamma_i;
		int r;
		leaf_offdiag(S, k, m, i0, gamma_i, r);
		bool nothing = false;
		if (k + 1 == m || gamma_i == (T) 0) {
			nothing = true;
		} else if (fabs(S[i0 * LB_LDP + i0]) >= alpha * gamma_i) {
			npiv = 1;
		} else {
			i1 = r;
			if (rook) {
				for (int it = 0;; ++it) { // (the cap only matters for non-finite input)
					T gamma_r;
					int s;
					leaf_offdiag(S, k, m, i1, gamma_r, s);
					if (fabs(S[i1 * LB_LDP + i1]) >= alpha * gamma_r) {
						npiv = 1;
						i0 = i1;
						break;
					} else if (s == i0 || gamma_i == gamma_r || it >= m) {
						npiv = 2;
						break;
					} else {
						i0 = i1;
						i1 = s;
						gamma_i = gamma_r;
					}
				}
			} else {
				T gamma_r;
				int s;
				leaf_offdiag(S, k, m, i1, gamma_r, s);
				if (fabs(S[i0 * LB_LDP + i0]) >= (alpha * gamma_r) * (gamma_r / gamma_i)) {
					npiv = 1;
				} else if (fabs(S[i1 * LB_LDP + i1]) >= alpha * gamma_r) {
					npiv = 1;
					i0 = i1;
				} else {
					npiv = 2;
				}
			}
		}
		if (npiv == 2 && i0 > i1) {
			const int t = i0;
			i0 = i1;
			i1 = t;
		}
		__syncthreads();
		if (i0 != k)
			leaf_sym_swap(S, m, k, i0);
		if (npiv == 2 && i1 != k + 1)
			leaf_sym_swap(S, m, k + 1, i1);
		if (nothing) {
			if (tid == 0) {
				s_sub[k] = (T) 0;
				s_piv[k] = i0;
			}
		} else if (npiv == 1) {
			leaf_eliminate_1x1(S, k, m);
			if (tid == 0) {
				s_sub[k] = (T) 0;
				s_piv[k] = i0;
			}
		} else {
			const T a10 = leaf_eliminate_2x2(S, k, m);
			if (tid == 0) {
				S[k * LB_LDP + k + 1] = (T) 0;
				s_sub[k] = a10;
				s_sub[k + 1] = (T) 0;
				s_piv[k] = i0;
				s_piv[k + 1] = i1;
			}
			++n2;
		}
		k += npiv;
	}
	__syncthreads();
	for (int e = tid; e < m * m; e += LB_NT) {
		const int i = e % m, j = e / m;
		if (j <= i)
			A[(idx_t) i * rs + (idx_t) j * cs] = S[j * LB_LDP + i];
	}
	if (tid < m) {
		sub[(idx_t) tid * ss] = s_sub[tid];
		piv[tid] = s_piv[tid];
	}
	if (tid == 0)
		st[ST_N2X2] += n2;
}

// ------------------------------------------------------------------------------------------------ panel
// start of a panel on the m x m trailing block Ab: k = 0 and the first diagonal arg-max
template <typename T> __global__ __launch_bounds__(LB_PT) void lblt_panel_init_kernel(const T *Ab, idx_t rs, idx_t cs, int m, int *st, int diagonal)
{
	__shared__ T s_v[LB_PT / 64];
	__shared__ int s_i[LB_PT / 64];
	const int tid = threadIdx.x;
	int i0 = 0;
	if (diagonal) {
		T v = (T) -1;
		i0 = LB_NOIDX;
		for (int r = tid; r < m; r += LB_PT) {
			const T x = fabs(Ab[(idx_t) r * (rs + cs)]);
			if (x > v) {
				v = x;
				i0 = r;
			}
		}
		block_argmax<T, LB_PT>(v, i0, s_v, s_i);
		if (i0 == LB_NOIDX)
			i0 = 0;
	}
	if (tid == 0) {
		st[ST_K] = 0;
		st[ST_DONE] = 0;
		st[ST_I0] = i0;
		st[ST_I1] = 0;
		st[ST_NEED2] = 0;
		st[ST_NOTHING] = 0;
		st[ST_AGAIN] = 0;
	}
}

// Candidate column of the lazily updated trailing matrix: W[:, k + which] = a(:, idx) - A_l W_l[idx, :]^T over the rows k .. m - 1, with
// the current diagonal entry at row idx, and this workgroup's arg-max candidate of the off-diagonal part.  which == 0: idx = i0.
// which == 1: idx = i1 -- with from_state == 0 every workgroup first takes the decision "is a second column needed" from the first pass's
// candidates (workgroup 0 records it for the pivot kernel); with from_state == 1 (a further rook iteration) the state says so.
template <typename T>
__global__ __launch_bounds__(LB_NT) void lblt_col_kernel(const T *Ab, idx_t rs, idx_t cs, int m, T *W, int *st, T *fv, Cand<T> *cands, int nwg,
							  int which, int from_state)
{
	__shared__ T s_v[LB_NT / 64];
	__shared__ int s_i[LB_NT / 64];
	__shared__ T s_w[LB_NB];
	if (st[ST_DONE])
		return;
	const int tid = threadIdx.x;
	const int k = st[ST_K];
	int idx;
	if (which == 0) {
		idx = st[ST_I0];
	} else if (from_state) {
		if (!st[ST_AGAIN])
			return;
		idx = st[ST_I1];
	} else {
		const int i0 = st[ST_I0];
		T g = (T) -1;
		int r = LB_NOIDX;
		for (int w = tid; w < nwg; w += LB_NT) { // (ascending w: ascending rows)
			const Cand<T> c = cands[w];
			if (c.v > g || (c.v == g && c.i < r)) {
				g = c.v;
				r = c.i;
			}
		}
		block_argmax<T, LB_NT>(g, r, s_v, s_i);
		const bool nothing = g == (T) 0 || r == LB_NOIDX; // (no index: non-finite input)
		const bool need2 = !nothing && !(fabs(Ab[(idx_t) i0 * (rs + cs)]) >= lb_alpha<T>() * g);
		if (blockIdx.x == 0 && tid == 0) {
			st[ST_NEED2] = need2;
			st[ST_NOTHING] = nothing;
			st[ST_I1] = r;
			fv[0] = g;
		}
		if (!need2)
			return;
		idx = r;
	}
	if (tid < k)
		s_w[tid] = W[idx + (idx_t) tid * m];
	__syncthreads();
	const int r = blockIdx.x * LB_NT + tid;
	T v = (T) -1;
	int vi = LB_NOIDX;
	if (r >= k && r < m) {
		T acc;
		if (r == idx) {
			acc = Ab[(idx_t) idx * (rs + cs)];
		} else {
			acc = r < idx ? Ab[(idx_t) idx * rs + (idx_t) r * cs] : Ab[(idx_t) r * rs + (idx_t) idx * cs];
			const T *al = Ab + (idx_t) r * rs;
			for (int j = 0; j < k; ++j)
				acc = fh_fma(-al[(idx_t) j * cs], s_w[j], acc);
			v = fabs(acc);
			vi = r;
		}
		W[r + (idx_t) (k + which) * m] = acc;
	}
	block_argmax<T, LB_NT>(v, vi, s_v, s_i);
	if (tid == 0) {
		Cand<T> c;
		c.v = v;
		c.i = vi;
		cands[which * nwg + blockIdx.x] = c;
	}
}

// swap of the indices a < b of the symmetric matrix stored in the lower triangle of Ab, restricted to the trailing part that starts at
// column k (factor.rs:37-53), together with the rows a, b of the panel's L columns (0 .. k - 1) and of the first wc columns of W
template <typename T>
static __device__ __forceinline__ void panel_sym_swap(T *Ab, idx_t rs, idx_t cs, int m, T *W, int wc, int a, int b)
{
	const int tid = threadIdx.x;
	for (int r = b + 1 + tid; r < m; r += LB_PT) { // columns a, b below row b
		T *p = Ab + (idx_t) r * rs;
		const T x = p[(idx_t) a * cs];
		p[(idx_t) a * cs] = p[(idx_t) b * cs];
		p[(idx_t) b * cs] = x;
	}
	for (int c = tid; c < a; c += LB_PT) { // rows a, b left of column a (the panel's L columns and the trailing columns before a)
		T *p = Ab + (idx_t) c * cs;
		const T x = p[(idx_t) a * rs];
		p[(idx_t) a * rs] = p[(idx_t) b * rs];
		p[(idx_t) b * rs] = x;
	}
	for (int t = a + 1 + tid; t < b; t += LB_PT) { // column a between the rows <-> row b between the columns
		T *p = Ab + (idx_t) t * rs + (idx_t) a * cs, *q = Ab + (idx_t) b * rs + (idx_t) t * cs;
		const T x = *p;
		*p = *q;
		*q = x;
	}
	for (int c = tid; c < wc; c += LB_PT) {
		T *p = W + (idx_t) c * m;
		const T x = p[a];
		p[a] = p[b];
		p[b] = x;
	}
	if (tid == 0) {
		T *p = Ab + (idx_t) a * (rs + cs), *q = Ab + (idx_t) b * (rs + cs);
		const T x = *p;
		*p = *q;
		*q = x;
	}
	__syncthreads();
}

// One workgroup: final decision of the step, swaps, elimination, pivot record, next diagonal arg-max (factor.rs:543-679).
// sub: the panel's part of subdiag; piv: its pivot rows, relative to the block.
template <typename T>
__global__ __launch_bounds__(LB_PT) void lblt_pivot_kernel(T *Ab, idx_t rs, idx_t cs, int m, T *W, int *st, T *fv, const Cand<T> *cands, int nwg,
							    T *sub, idx_t ss, int *piv, int rook, int diagonal)
{
	__shared__ T s_v[LB_PT / 64];
	__shared__ int s_i[LB_PT / 64];
	if (st[ST_DONE])
		return;
	const int tid = threadIdx.x;
	const T alpha = lb_alpha<T>();
	const int k = st[ST_K];
	int i0 = st[ST_I0], i1 = st[ST_I1];
	const bool nothing = st[ST_NOTHING] != 0, need2 = st[ST_NEED2] != 0;
	const T gamma_i = fv[0];
	int npiv = 1;
	bool use1 = false; // the pivot column is the second candidate column
	__syncthreads();   // every thread has read the state before thread 0 rewrites it
	if (!nothing && need2) {
		T gamma_r = (T) -1;
		int s = LB_NOIDX;
		for (int w = tid; w < nwg; w += LB_PT) {
			const Cand<T> c = cands[nwg + w];
			if (c.v > gamma_r || (c.v == gamma_r && c.i < s)) {
				gamma_r = c.v;
				s = c.i;
			}
		}
		block_argmax<T, LB_PT>(gamma_r, s, s_v, s_i);
		const T d0 = fabs(Ab[(idx_t) i0 * (rs + cs)]), d1 = fabs(Ab[(idx_t) i1 * (rs + cs)]);
		if (!rook) {
			if (d0 >= (alpha * gamma_r) * (gamma_r / gamma_i)) {
				npiv = 1;
			} else if (d1 >= alpha * gamma_r) {
				npiv = 1;
				i0 = i1;
				use1 = true;
			} else {
				npiv = 2;
			}
		} else {
			if (d1 >= alpha * gamma_r) {
				npiv = 1;
				i0 = i1;
				use1 = true;
			} else if (s == i0 || gamma_i == gamma_r || s == LB_NOIDX) {
				npiv = 2;
			} else { // one more rook iteration: (i0, i1, gamma_i) <- (i1, s, gamma_r), the second column becomes the first
				for (int r = k + tid; r < m; r += LB_PT)
					W[r + (idx_t) k * m] = W[r + (idx_t) (k + 1) * m];
				if (tid == 0) {
					st[ST_I0] = i1;
					st[ST_I1] = s;
					fv[0] = gamma_r;
					st[ST_AGAIN] = 1;
				}
				return;
			}
		}
	}
	if (use1) {
		for (int r = k + tid; r < m; r += LB_PT)
			W[r + (idx_t) k * m] = W[r + (idx_t) (k + 1) * m];
	}
	if (npiv == 2 && i0 > i1) {
		for (int r = k + tid; r < m; r += LB_PT) {
			const T x = W[r + (idx_t) k * m];
			W[r + (idx_t) k * m] = W[r + (idx_t) (k + 1) * m];
			W[r + (idx_t) (k + 1) * m] = x;
		}
		const int t = i0;
		i0 = i1;
		i1 = t;
	}
	__syncthreads();
	if (i0 != k)
		panel_sym_swap(Ab, rs, cs, m, W, k + npiv, k, i0);
	if (npiv == 2 && i1 != k + 1)
		panel_sym_swap(Ab, rs, cs, m, W, k + npiv, k + 1, i1);
	const T *w0p = W + (idx_t) k * m, *w1p = W + (idx_t) (k + 1) * m;
	if (nothing) {
		// the updated column is zero below the diagonal: that is the L column (the stored one is not up to date)
		for (int r = k + 1 + tid; r < m; r += LB_PT)
			Ab[(idx_t) r * rs + (idx_t) k * cs] = w0p[r];
		if (tid == 0)
			sub[(idx_t) k * ss] = (T) 0;
	} else if (npiv == 1) {
		const T diag = w0p[k];
		const T dinv = (T) 1 / diag;
		for (int r = k + 1 + tid; r < m; r += LB_PT) {
			const T l = w0p[r] * dinv;
			Ab[(idx_t) r * rs + (idx_t) k * cs] = l;
			T *dd = Ab + (idx_t) r * (rs + cs);
			*dd = *dd - diag * (l * l);
		}
		if (tid == 0)
			sub[(idx_t) k * ss] = (T) 0;
	} else {
		const T a00 = w0p[k], a11 = w1p[k + 1], a10 = w0p[k + 1];
		const T d10_inv = (T) 1 / fabs(a10);
		const T d00 = a00 * d10_inv, d11 = a11 * d10_inv;
		const T t = (T) 1 / (d00 * d11 - (T) 1);
		const T d10 = a10 * d10_inv;
		const T d = t * d10_inv;
		__syncthreads(); // a10 is read by every thread before thread 0 clears it
		for (int r = k + 2 + tid; r < m; r += LB_PT) {
			const T x0 = w0p[r], x1 = w1p[r];
			const T w0 = (x0 * d11 - x1 * d10) * d;
			const T w1 = (x1 * d00 - x0 * d10) * d;
			T *dd = Ab + (idx_t) r * (rs + cs);
			*dd = *dd - x0 * w0 - x1 * w1;
			Ab[(idx_t) r * rs + (idx_t) k * cs] = w0;
			Ab[(idx_t) r * rs + (idx_t) (k + 1) * cs] = w1;
		}
		if (tid == 0) {
			sub[(idx_t) k * ss] = a10;
			sub[(idx_t) (k + 1) * ss] = (T) 0;
			W[(k + 1) + (idx_t) k * m] = (T) 0;
			Ab[(idx_t) (k + 1) * rs + (idx_t) k * cs] = (T) 0;
		}
	}
	const int knew = k + npiv;
	__syncthreads();
	int inext = knew;
	if (diagonal) {
		T v = (T) -1;
		inext = LB_NOIDX;
		for (int r = knew + tid; r < m; r += LB_PT) {
			const T x = fabs(Ab[(idx_t) r * (rs + cs)]);
			if (x > v) {
				v = x;
				inext = r;
			}
		}
		block_argmax<T, LB_PT>(v, inext, s_v, s_i);
		if (inext == LB_NOIDX)
			inext = knew;
	}
	if (tid == 0) {
		piv[k] = i0;
		if (npiv == 2) {
			piv[k + 1] = i1;
			st[ST_N2X2] += 1;
		}
		st[ST_K] = knew;
		st[ST_DONE] = knew >= LB_NB - 1;
		st[ST_I0] = inext;
		st[ST_NEED2] = 0;
		st[ST_NOTHING] = 0;
		st[ST_AGAIN] = 0;
	}
}

// ------------------------------------------------------------------------------------------------ Full
// Full pivoting (factor.rs:264-429, lblt_full_piv): an unblocked level-2 algorithm.  The lower triangle is scaled by the reciprocal of
// its largest magnitude; every step takes the largest diagonal entry as a 1 x 1 pivot if its square is at least alpha^2 times the
// largest squared off-diagonal entry of the trailing matrix, else that off-diagonal entry as a 2 x 2 pivot; once the trailing
// off-diagonal is zero the remaining diagonal is only sorted (the tail).  Two launches per step and no host synchronisation inside:
//   lblt_full_pivot_kernel  (one workgroup) combines the candidates of the previous pass, finds the diagonal arg-max, decides, swaps,
//                           forms L, the w vectors and the trailing diagonal, records the pivot and advances k in the device state;
//   lblt_full_update_kernel (64 x 64 tiles on or below the diagonal of the trailing matrix, lanes along the rows) applies the rank-1 /
//                           rank-2 update to the strict lower triangle and takes the arg-max of a^2 in the same pass, one candidate
//                           per tile.
// The host only knows a lower bound of k: it sizes the grid for the largest trailing matrix still possible, surplus tiles and surplus
// steps return on the device state, and it reads (k, done) back once per 64 launched steps.  The last <= 64 rows, tail included, are
// finished by one LDS-resident workgroup (lblt_full_leaf_kernel), which recomputes the off-diagonal arg-max from its image.
// Ties: the largest value, then the lowest column, then the lowest row (the reference's column-major scan with a strict >).
constexpr int LF_T = 64;   // tile edge: 256 threads, lane = row, 16 columns per wavefront
constexpr int LF_CPW = 16; // columns per wavefront
constexpr long long LF_NOKEY = 0x7fffffffffffffffLL;
enum { FS_NPIV = 8, FS_TAIL, FS_STEPS, FS_KLEAF }; // device state of the Full path, after ST_N2X2
enum { FV_SCALE = 0, FV_INV, FV_D };		   // fv: the scale, its reciprocal, the 1 x 1 pivot of the current step
enum { LF_ABSMAX = 0, LF_RANK1 = 1, LF_RANK2 = 2, LF_SCALE = 3 };

// candidate of one tile: squared magnitude (LF_ABSMAX: magnitude) and (column << 32) | row, both relative to the trailing matrix
template <typename T> struct FCand {
	T v;
	long long key;
};

// One 64 x 64 tile of the trailing lower triangle that starts at row / column kt.  Tiles on or below the diagonal only: grid row y
// holds tile row y and, behind it, tile row nt - 1 - y (nt + 1 tiles together).  wv: the vectors of the pivot kernel, n entries
// each, indexed by the absolute row -- rank 1: l; rank 2: x0, x1, w0, w1.
//   LF_ABSMAX: candidate = largest |a|, diagonal included, nothing written       LF_SCALE: a *= fv[FV_INV], diagonal included
//   LF_RANK1:  a_ij -= (l_i l_j) d                                                LF_RANK2: a_ij -= x0_i w0_j + x1_i w1_j
// and for the last three the candidate = first largest a^2 of the strict lower triangle.
template <typename T, int MODE>
static __device__ __forceinline__ void full_tile(T *A, idx_t rs, idx_t cs, int n, int kt, const T *fv, const T *wv, FCand<T> *cands)
{
	__shared__ T s_v[LB_NT / 64];
	__shared__ long long s_k[LB_NT / 64];
	const int mt = n - kt, nt = (mt + LF_T - 1) / LF_T;
	const int gx = blockIdx.x, gy = blockIdx.y;
	if (gy >= (nt + 1) / 2 || gx > nt)
		return; // the grid was sized for a larger trailing matrix
	int bi, bj;
	if (gx <= gy) {
		bi = gy;
		bj = gx;
	} else {
		bi = nt - 1 - gy;
		bj = gx - gy - 1;
		if (bi == gy)
			return; // odd nt: the middle tile row is alone in its grid row
	}
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int il = bi * LF_T + lane, jl0 = bj * LF_T + wave * LF_CPW;
	const bool with_diag = MODE == LF_ABSMAX || MODE == LF_SCALE;
	T x0 = (T) 0, x1 = (T) 0;
	if (MODE == LF_RANK1 || MODE == LF_RANK2)
		x0 = il < mt ? wv[kt + il] : (T) 0;
	if (MODE == LF_RANK2)
		x1 = il < mt ? wv[(idx_t) n + kt + il] : (T) 0;
	const T sc = MODE == LF_SCALE ? fv[FV_INV] : (MODE == LF_RANK1 ? fv[FV_D] : (T) 0);
	T *row = A + (idx_t) (kt + il) * rs + (idx_t) kt * cs;
	// every element of the thread is loaded before the first store
	T a[LF_CPW], w0[LF_CPW], w1[LF_CPW];
#pragma unroll
	for (int c = 0; c < LF_CPW; ++c) {
		const int jl = jl0 + c;
		const bool ok = il < mt && (with_diag ? jl <= il : jl < il);
		a[c] = ok ? row[(idx_t) jl * cs] : (T) 0;
		const int jc = min(kt + jl, n - 1); // (uniform per wavefront; clamped: always in bounds)
		w0[c] = MODE == LF_RANK1 ? wv[jc] : (MODE == LF_RANK2 ? wv[(idx_t) 2 * n + jc] : (T) 0);
		w1[c] = MODE == LF_RANK2 ? wv[(idx_t) 3 * n + jc] : (T) 0;
	}
	T bv = (T) 0;
	long long bk = LF_NOKEY;
#pragma unroll
	for (int c = 0; c < LF_CPW; ++c) {
		const int jl = jl0 + c;
		const bool ok = il < mt && (with_diag ? jl <= il : jl < il);
		if (!ok)
			continue;
		T v = a[c];
		if (MODE == LF_RANK1)
			v = v - (x0 * w0[c]) * sc;
		if (MODE == LF_RANK2)
			v = v - x0 * w0[c] - x1 * w1[c];
		if (MODE == LF_SCALE)
			v = v * sc;
		if (MODE != LF_ABSMAX)
			row[(idx_t) jl * cs] = v;
		const T q = MODE == LF_ABSMAX ? fabs(v) : (jl < il ? v * v : (T) 0);
		if (q > bv) { // (ascending columns: the first maximum of the row)
			bv = q;
			bk = ((long long) jl << 32) | (long long) il;
		}
	}
	block_argmax<T, LB_NT>(bv, bk, s_v, s_k);
	if (tid == 0) {
		FCand<T> cd;
		cd.v = bv;
		cd.key = bk;
		cands[(size_t) bi * (bi + 1) / 2 + bj] = cd;
	}
}

// the two passes in front of the loop, over the whole lower triangle: LF_ABSMAX, then LF_SCALE with the first arg-max
template <typename T, int MODE>
__global__ __launch_bounds__(LB_NT) void lblt_full_prep_kernel(T *A, idx_t rs, idx_t cs, int n, const T *fv, FCand<T> *cands)
{
	full_tile<T, MODE>(A, rs, cs, n, 0, fv, (const T *) nullptr, cands);
}

// scale = the largest magnitude of the lower triangle from the LF_ABSMAX candidates.  A zero matrix (and one without a finite
// positive maximum) is not scaled: both factors are 1.
template <typename T> __global__ __launch_bounds__(LB_PT) void lblt_full_scale_kernel(const FCand<T> *cands, int nc, T *fv)
{
	__shared__ T s_v[LB_PT / 64];
	__shared__ int s_i[LB_PT / 64];
	T v = (T) 0;
	int i = 0;
	for (int w = threadIdx.x; w < nc; w += LB_PT) {
		const T x = cands[w].v;
		if (x > v)
			v = x;
	}
	block_argmax<T, LB_PT>(v, i, s_v, s_i);
	if (threadIdx.x == 0) {
		const bool scaled = v > (T) 0;
		fv[FV_SCALE] = scaled ? v : (T) 1;
		fv[FV_INV] = scaled ? (T) 1 / v : (T) 1;
		fv[FV_D] = (T) 0;
	}
}

// the strict lower triangle of the trailing matrix behind the pivot the pivot kernel has just taken
template <typename T>
__global__ __launch_bounds__(LB_NT) void lblt_full_update_kernel(T *A, idx_t rs, idx_t cs, int n, const int *st, const T *fv, const T *wv,
								  FCand<T> *cands)
{
	if (st[ST_DONE])
		return;
	const int npiv = st[FS_NPIV], kt = st[ST_K];
	if (npiv == 1)
		full_tile<T, LF_RANK1>(A, rs, cs, n, kt, fv, wv, cands);
	else if (npiv == 2)
		full_tile<T, LF_RANK2>(A, rs, cs, n, kt, fv, wv, cands);
	// (0: the tail, or the rows left belong to the leaf)
}

// One workgroup per step (factor.rs:295-425).  A: the whole matrix; sub, piv: whole vectors, absolute pivot rows.
template <typename T>
__global__ __launch_bounds__(LB_PT) void lblt_full_pivot_kernel(T *A, idx_t rs, idx_t cs, int n, int *st, T *fv, T *wv, const FCand<T> *cands,
								 T *sub, idx_t ss, int *piv)
{
	__shared__ T s_v[LB_PT / 64];
	__shared__ long long s_k[LB_PT / 64];
	__shared__ int s_i[LB_PT / 64];
	if (st[ST_DONE])
		return;
	const int tid = threadIdx.x;
	const int k = st[ST_K], m = n - k;
	bool tail = st[FS_TAIL] != 0;
	__syncthreads(); // every thread has read the state before thread 0 rewrites it
	if (m <= LB_NB) { // the leaf takes over
		if (tid == 0) {
			st[ST_DONE] = 1;
			st[FS_NPIV] = 0;
		}
		return;
	}
	T mo = (T) 0;
	long long key = LF_NOKEY;
	if (!tail) {
		const int nt = (m + LF_T - 1) / LF_T, nc = nt * (nt + 1) / 2;
		for (int w = tid; w < nc; w += LB_PT) {
			const FCand<T> c = cands[w];
			if (c.v > mo || (c.v == mo && c.key < key)) {
				mo = c.v;
				key = c.key;
			}
		}
		block_argmax<T, LB_PT>(mo, key, s_v, s_k);
		if (!(mo > (T) 0) || key == LF_NOKEY)
			tail = true;
	}
	T md = (T) -1;
	int ms = LB_NOIDX;
	for (int r = tid; r < m; r += LB_PT) {
		const T x = A[(idx_t) (k + r) * (rs + cs)];
		const T q = x * x;
		if (q > md) {
			md = q;
			ms = r;
		}
	}
	block_argmax<T, LB_PT>(md, ms, s_v, s_i);
	if (ms == LB_NOIDX) { // (non-finite input)
		ms = 0;
		md = (T) 0;
	}
	if (tail) { // factor.rs:402-425: the diagonal entries and the rows of the columns on the left change places, nothing is eliminated
		if (ms != 0) {
			T *pa = A + (idx_t) k * rs, *pb = A + (idx_t) (k + ms) * rs;
			for (int c = tid; c < k; c += LB_PT) {
				const T x = pa[(idx_t) c * cs];
				pa[(idx_t) c * cs] = pb[(idx_t) c * cs];
				pb[(idx_t) c * cs] = x;
			}
			if (tid == 0) {
				T *p = A + (idx_t) k * (rs + cs), *q = A + (idx_t) (k + ms) * (rs + cs);
				const T x = *p;
				*p = *q;
				*q = x;
			}
		}
		if (tid == 0) {
			sub[(idx_t) k * ss] = (T) 0;
			piv[k] = k + ms;
			st[ST_K] = k + 1;
			st[FS_NPIV] = 0;
			st[FS_TAIL] = 1;
			st[FS_STEPS] += 1;
		}
		return;
	}
	const T alpha = lb_alpha<T>() * lb_alpha<T>();
	const int mi = (int) (key & 0xffffffffLL), mj = (int) (key >> 32);
	int npiv = 2, i0 = mj, i1 = mi;
	if (md >= alpha * mo || !(mj < mi && mi < m)) { // (the second test never holds: candidates name entries of the strict lower triangle)
		npiv = 1;
		i0 = ms;
	}
	if (i0 != 0)
		panel_sym_swap(A, rs, cs, n, (T *) nullptr, 0, k, k + i0);
	if (npiv == 2 && i1 != 1)
		panel_sym_swap(A, rs, cs, n, (T *) nullptr, 0, k + 1, k + i1);
	if (npiv == 1) {
		const T d = A[(idx_t) k * (rs + cs)];
		const T dinv = (T) 1 / d;
		for (int r = k + 1 + tid; r < n; r += LB_PT) {
			T *p = A + (idx_t) r * rs + (idx_t) k * cs;
			const T l = *p * dinv;
			*p = l;
			wv[r] = l;
			T *dd = A + (idx_t) r * (rs + cs);
			*dd = *dd - d * (l * l);
		}
		if (tid == 0) {
			fv[FV_D] = d;
			sub[(idx_t) k * ss] = (T) 0;
		}
	} else {
		T *p10 = A + (idx_t) (k + 1) * rs + (idx_t) k * cs;
		const T a00 = A[(idx_t) k * (rs + cs)], a11 = A[(idx_t) (k + 1) * (rs + cs)], a10 = *p10;
		const T d10_inv = (T) 1 / fabs(a10);
		const T d00 = a00 * d10_inv, d11 = a11 * d10_inv;
		const T t = (T) 1 / (d00 * d11 - (T) 1);
		const T d10 = a10 * d10_inv;
		const T d = t * d10_inv;
		__syncthreads(); // a10 is read by every thread before thread 0 clears it
		for (int r = k + 2 + tid; r < n; r += LB_PT) {
			T *p0 = A + (idx_t) r * rs + (idx_t) k * cs, *p1 = p0 + cs;
			const T x0 = *p0, x1 = *p1;
			const T w0 = (x0 * d11 - x1 * d10) * d;
			const T w1 = (x1 * d00 - x0 * d10) * d;
			T *dd = A + (idx_t) r * (rs + cs);
			*dd = *dd - x0 * w0 - x1 * w1;
			*p0 = w0;
			*p1 = w1;
			wv[r] = x0;
			wv[(idx_t) n + r] = x1;
			wv[(idx_t) 2 * n + r] = w0;
			wv[(idx_t) 3 * n + r] = w1;
		}
		if (tid == 0) {
			sub[(idx_t) k * ss] = a10;
			sub[(idx_t) (k + 1) * ss] = (T) 0;
			*p10 = (T) 0;
		}
	}
	if (tid == 0) {
		piv[k] = k + i0;
		if (npiv == 2) {
			piv[k + 1] = k + i1;
			st[ST_N2X2] += 1;
		}
		st[ST_K] = k + npiv;
		st[FS_NPIV] = npiv;
		st[FS_STEPS] += 1;
	}
}

// The rows from k = st[ST_K] on, at most 64: main loop and tail on the full symmetric image in LDS, with the swap and elimination
// helpers of lblt_leaf_kernel; then the leaf's transpositions on the columns left of it.
template <typename T>
__global__ __launch_bounds__(LB_NT) void lblt_full_leaf_kernel(T *A0, idx_t rs, idx_t cs, int n, T *sub0, idx_t ss, int *piv0, int *st)
{
	__shared__ T S[LB_NB * LB_LDP];
	__shared__ T s_sub[LB_NB];
	__shared__ int s_piv[LB_NB];
	__shared__ T s_v[LB_NT / 64];
	__shared__ int s_i[LB_NT / 64];
	const int tid = threadIdx.x, lane = tid & 63;
	const int k0 = st[ST_K], m = n - k0;
	if (m > LB_NB || m <= 0)
		return; // (the driver launches enough steps: never)
	T *A = A0 + (idx_t) k0 * (rs + cs);
	const T alpha = lb_alpha<T>() * lb_alpha<T>();
	for (int e = tid; e < m * m; e += LB_NT) {
		const int i = e % m, j = e / m;
		S[j * LB_LDP + i] = j <= i ? A[(idx_t) i * rs + (idx_t) j * cs] : A[(idx_t) j * rs + (idx_t) i * cs];
	}
	int n2 = 0;
	int k = 0;
	while (k < m) {
		__syncthreads();
		// first largest a^2 of the trailing strict lower triangle, column major; key = column * 64 + row
		const int mm = m - k;
		T mo = (T) 0;
		int key = LB_NOIDX;
		for (int e = tid; e < mm * mm; e += LB_NT) {
			const int i = k + e % mm, j = k + e / mm;
			if (i <= j)
				continue;
			const T x = S[j * LB_LDP + i];
			const T q = x * x;
			if (q > mo) {
				mo = q;
				key = j * LB_NB + i;
			}
		}
		block_argmax<T, LB_NT>(mo, key, s_v, s_i);
		// first largest a^2 of the trailing diagonal: every wavefront by itself (a NaN never wins)
		T md = (T) -1;
		if (lane >= k && lane < m) {
			const T x = S[lane * LB_LDP + lane];
			const T q = x * x;
			md = q >= (T) 0 ? q : (T) -1;
		}
		int ms = lane;
		wave_argmax(md, ms);
		if (md < (T) 0) {
			ms = k;
			md = (T) 0;
		}
		if (!(mo > (T) 0) || key == LB_NOIDX) { // the tail
			__syncthreads(); // every wavefront has read the diagonal
			if (ms != k) {
				if (tid < k) {
					const T x = S[tid * LB_LDP + k];
					S[tid * LB_LDP + k] = S[tid * LB_LDP + ms];
					S[tid * LB_LDP + ms] = x;
				}
				if (tid == 0) {
					const T x = S[k * LB_LDP + k];
					S[k * LB_LDP + k] = S[ms * LB_LDP + ms];
					S[ms * LB_LDP + ms] = x;
				}
			}
			if (tid == 0) {
				s_sub[k] = (T) 0;
				s_piv[k] = ms;
			}
			k += 1;
			continue;
		}
		int npiv = 2, i0 = key / LB_NB, i1 = key % LB_NB;
		if (md >= alpha * mo) {
			npiv = 1;
			i0 = ms;
		}
		__syncthreads();
		if (i0 != k)
			leaf_sym_swap(S, m, k, i0);
		if (npiv == 2 && i1 != k + 1)
			leaf_sym_swap(S, m, k + 1, i1);
		if (npiv == 1) {
			leaf_eliminate_1x1(S, k, m);
			if (tid == 0) {
				s_sub[k] = (T) 0;
				s_piv[k] = i0;
			}
		} else {
			const T a10 = leaf_eliminate_2x2(S, k, m);
			if (tid == 0) {
				S[k * LB_LDP + k + 1] = (T) 0;
				s_sub[k] = a10;
				s_sub[k + 1] = (T) 0;
				s_piv[k] = i0;
				s_piv[k + 1] = i1;
			}
			++n2;
		}
		k += npiv;
	}
	__syncthreads();
	for (int e = tid; e < m * m; e += LB_NT) {
		const int i = e % m, j = e / m;
		if (j <= i)
			A[(idx_t) i * rs + (idx_t) j * cs] = S[j * LB_LDP + i];
	}
	if (tid < m) {
		sub0[(idx_t) (k0 + tid) * ss] = s_sub[tid];
		piv0[k0 + tid] = k0 + s_piv[tid];
	}
	for (int c = tid; c < k0; c += LB_NT) { // one thread per column on the left: the m transpositions in order
		T *col = A0 + (idx_t) k0 * rs + (idx_t) c * cs;
		for (int t = 0; t < m; ++t) {
			const int p = s_piv[t];
			if (p != t) {
				const T x = col[(idx_t) t * rs];
				col[(idx_t) t * rs] = col[(idx_t) p * rs];
				col[(idx_t) p * rs] = x;
			}
		}
	}
	if (tid == 0) {
		st[ST_N2X2] += n2;
		st[FS_KLEAF] = k0;
	}
}

// the diagonal of B and subdiag go back to the scale of the input; L has none
template <typename T> __global__ void lblt_full_unscale_kernel(T *A, idx_t rs, idx_t cs, int n, T *sub, idx_t ss, const T *fv)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const T sc = fv[FV_SCALE];
	T *d = A + (idx_t) i * (rs + cs);
	*d = *d * sc;
	sub[(idx_t) i * ss] = sub[(idx_t) i * ss] * sc;
}

// panels, leaf rows, 2 x 2 pivots, host synchronisations inside panels (Full: pivot steps of the multi-workgroup path, leaf rows,
// 2 x 2 pivots, host synchronisations before the leaf)
thread_local size_t g_last[4] = {0, 0, 0, 0};

// reads `cnt` ints of the device state back (one host synchronisation)
void read_state(const int *st, int *out, int first, int cnt)
{
	int *h = ctx().pinned_ints();
	FH_HIP(hipMemcpyAsync(h, st + first, (size_t) cnt * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
	ctx().sync();
	for (int i = 0; i < cnt; ++i)
		out[i] = h[i];
}

// Full pivoting on the buffers of lblt_dev: st (zeroed here), fv, piv (absolute pivot rows), cands (one per tile of the whole lower
// triangle), wv (4 n entries)
template <typename T>
long lblt_full_dev(MatV<T> A, T *sub, idx_t ss, idx_t *perm, idx_t *perm_inv, int *st, T *fv, int *piv, FCand<T> *cands, T *wv)
{
	const int n = (int) A.nrows;
	hipStream_t s = ctx().stream;
	auto tiles = [](int mt) { // the folded grid of the tile triangle of an mt x mt matrix
		const int nt = (mt + LF_T - 1) / LF_T;
		return dim3((unsigned) (nt + 1), (unsigned) ((nt + 1) / 2));
	};
	const int nt0 = (n + LF_T - 1) / LF_T;
	FH_HIP(hipMemsetAsync(st, 0, ST_COUNT * sizeof(int), s));
	hipLaunchKernelGGL((lblt_full_prep_kernel<T, LF_ABSMAX>), tiles(n), dim3(LB_NT), 0, s, A.p, A.rs, A.cs, n, fv, cands);
	hipLaunchKernelGGL(lblt_full_scale_kernel<T>, dim3(1), dim3(LB_PT), 0, s, cands, nt0 * (nt0 + 1) / 2, fv);
	hipLaunchKernelGGL((lblt_full_prep_kernel<T, LF_SCALE>), tiles(n), dim3(LB_NT), 0, s, A.p, A.rs, A.cs, n, fv, cands);
	// every launched step that is not past the hand-over advances k by 1 or 2: klo is the host's lower bound of k
	int klo = 0, since = 0;
	bool done = false;
	while (!done && n - klo > LB_NB) {
		hipLaunchKernelGGL(lblt_full_pivot_kernel<T>, dim3(1), dim3(LB_PT), 0, s, A.p, A.rs, A.cs, n, st, fv, wv, cands, sub, ss, piv);
		hipLaunchKernelGGL(lblt_full_update_kernel<T>, tiles(n - klo - 1), dim3(LB_NT), 0, s, A.p, A.rs, A.cs, n, st, fv, wv, cands);
		++klo;
		if (++since == 64 && n - klo > LB_NB) {
			int h[2];
			read_state(st, h, ST_K, 2); // ST_K, ST_DONE
			++g_last[3];
			klo = std::max(klo, h[0]);
			done = h[1] != 0;
			since = 0;
		}
	}
	hipLaunchKernelGGL(lblt_full_leaf_kernel<T>, dim3(1), dim3(LB_NT), 0, s, A.p, A.rs, A.cs, n, sub, ss, piv, st);
	hipLaunchKernelGGL(lblt_full_unscale_kernel<T>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, A.p, A.rs, A.cs, n, sub, ss, fv);
	FH_HIP(hipGetLastError());
	std::vector<int> hp((size_t) n);
	int h[ST_COUNT];
	FH_HIP(hipMemcpyAsync(hp.data(), piv, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, s));
	read_state(st, h, 0, ST_COUNT);
	FH_CHECK(n - h[FS_KLEAF] <= LB_NB && h[FS_KLEAF] == h[ST_K], "lblt: the Full path did not reach its leaf");
	g_last[0] = (size_t) h[FS_STEPS];
	g_last[1] = (size_t) (n - h[FS_KLEAF]);
	g_last[2] = (size_t) h[ST_N2X2];
	return perm_from_transpositions("lblt", n, n, [&](idx_t i) { return (idx_t) hp[(size_t) i]; }, perm, perm_inv);
}

// A: n x n device view, sub: device, stride ss.  perm / perm_inv: host, n entries.  Returns the transposition count.
template <typename T> long lblt_dev(MatV<T> A, T *sub, idx_t ss, idx_t *perm, idx_t *perm_inv, bool rook, bool diagonal, bool full)
{
	const idx_t n = A.nrows;
	g_last[0] = g_last[1] = g_last[2] = g_last[3] = 0;
	if (n == 0)
		return 0;
	FH_CHECK(n < ((idx_t) 1 << 30), "lblt: dimension too large");
	hipStream_t s = ctx().stream;
	const int nwg_max = (int) ((n + LB_NT - 1) / LB_NT);
	const size_t ntf = (size_t) ((n + LF_T - 1) / LF_T); // Full: one candidate per tile of the lower triangle, four vectors in wb
	Scratch stb(ST_COUNT * sizeof(int)), fvb(4 * sizeof(T)), pivb((size_t) n * sizeof(int)),
		cab(full ? ntf * (ntf + 1) / 2 * sizeof(FCand<T>) : (size_t) 2 * nwg_max * sizeof(Cand<T>));
	Scratch wb(full ? (size_t) 4 * n * sizeof(T) : (n > LB_NB ? (size_t) n * LB_NB * sizeof(T) : 256));
	if (full)
		return lblt_full_dev<T>(A, sub, ss, perm, perm_inv, stb.as<int>(), fvb.as<T>(), pivb.as<int>(), cab.as<FCand<T>>(), wb.as<T>());
	int *st = stb.as<int>(), *piv = pivb.as<int>();
	T *fv = fvb.as<T>(), *W = wb.as<T>();
	Cand<T> *cands = cab.as<Cand<T>>();
	FH_HIP(hipMemsetAsync(st, 0, ST_COUNT * sizeof(int), s));
	std::vector<idx_t> starts; // block starts: the pivot records are relative to them
	idx_t k0 = 0;
	while (n - k0 > LB_NB) {
		const int m = (int) (n - k0);
		const int nwg = (m + LB_NT - 1) / LB_NT;
		T *Ab = A.p + k0 * (A.rs + A.cs);
		T *subp = sub + k0 * ss;
		int *pv = piv + k0;
		hipLaunchKernelGGL(lblt_panel_init_kernel<T>, dim3(1), dim3(LB_PT), 0, s, Ab, A.rs, A.cs, m, st, (int) diagonal);
		for (int step = 0; step < LB_NB - 1; ++step) {
			hipLaunchKernelGGL(lblt_col_kernel<T>, dim3(nwg), dim3(LB_NT), 0, s, Ab, A.rs, A.cs, m, W, st, fv, cands, nwg, 0, 0);
			hipLaunchKernelGGL(lblt_col_kernel<T>, dim3(nwg), dim3(LB_NT), 0, s, Ab, A.rs, A.cs, m, W, st, fv, cands, nwg, 1, 0);
			hipLaunchKernelGGL(lblt_pivot_kernel<T>, dim3(1), dim3(LB_PT), 0, s, Ab, A.rs, A.cs, m, W, st, fv, cands, nwg, subp, ss, pv,
					   (int) rook, (int) diagonal);
			if (rook) { // the length of the rook loop depends on the data: one flag per iteration
				int h[2];
				for (int it = 0;; ++it) {
					read_state(st, h, ST_AGAIN, 1);
					++g_last[3];
					if (!h[0])
						break;
					FH_CHECK(it < m, "lblt: the rook search did not terminate (non-finite input?)");
					hipLaunchKernelGGL(lblt_col_kernel<T>, dim3(nwg), dim3(LB_NT), 0, s, Ab, A.rs, A.cs, m, W, st, fv, cands, nwg, 1, 1);
					hipLaunchKernelGGL(lblt_pivot_kernel<T>, dim3(1), dim3(LB_PT), 0, s, Ab, A.rs, A.cs, m, W, st, fv, cands, nwg, subp,
							   ss, pv, (int) rook, (int) diagonal);
				}
			}
		}
		FH_HIP(hipGetLastError());
		int ke;
		read_state(st, &ke, ST_K, 1); // 63 or 64
		FH_CHECK(ke == LB_NB - 1 || ke == LB_NB, "lblt: panel ended at an unexpected column");
		const idx_t mr = m - ke;
		MatV<T> Ablk{Ab, m, m, A.rs, A.cs};
		MatV<T> Wv{W, m, LB_NB, 1, m};
		// A_r(strict lower) -= W A_l^T (factor.rs:684-694); the diagonal is already up to date
		matmul_triangular_dev<T>(Ablk.sub(ke, ke, mr, mr), (int) FaerBlock_StrictTriangularLower, true, Wv.sub(ke, 0, mr, ke).c(),
					 (int) FaerBlock_Rectangular, Ablk.sub(ke, 0, mr, ke).t().c(), (int) FaerBlock_Rectangular, (T) -1);
		if (k0 > 0)
			laswp_rows_dev<T>(A.sub(k0, 0, m, k0), pv, ke); // factor.rs:748-779
		starts.push_back(k0);
		k0 += ke;
		++g_last[0];
	}
	{
		const int m = (int) (n - k0);
		hipLaunchKernelGGL(lblt_leaf_kernel<T>, dim3(1), dim3(LB_NT), 0, s, A.p + k0 * (A.rs + A.cs), A.rs, A.cs, m, sub + k0 * ss, ss, piv + k0,
				   st, (int) rook, (int) diagonal);
		FH_HIP(hipGetLastError());
		if (k0 > 0)
			laswp_rows_dev<T>(A.sub(k0, 0, m, k0), piv + k0, m);
		starts.push_back(k0);
		g_last[1] = (size_t) m;
	}
	std::vector<int> hp((size_t) n);
	int n2;
	FH_HIP(hipMemcpyAsync(hp.data(), piv, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, s));
	read_state(st, &n2, ST_N2X2, 1);
	g_last[2] = (size_t) n2;
	// factor.rs:1214-1227
	size_t b = 0; // the records are relative to the first row of their block
	auto record = [&](idx_t i) {
		while (b + 1 < starts.size() && starts[b + 1] <= i)
			++b;
		return starts[b] + (idx_t) hp[(size_t) i];
	};
	return perm_from_transpositions("lblt", n, n, record, perm, perm_inv);
}

// ------------------------------------------------------------------------------------------------ solve / reconstruct
// x <- B^-1 x for the block diagonal B (solve.rs:63-96): one thread per (block, right-hand side)
template <typename T>
__global__ void lblt_block_diag_solve_kernel(T *X, idx_t rs, idx_t cs, idx_t n, idx_t k, const T *d, idx_t ds, const T *sub, idx_t ss)
{
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
	if (i >= n || j >= k)
		return;
	if (i > 0 && sub[(i - 1) * ss] != (T) 0)
		return; // second row of a 2 x 2 block
	T *x = X + i * rs + j * cs;
	const T s = sub[i * ss];
	if (s == (T) 0 || i + 1 >= n) {
		*x = *x * ((T) 1 / d[i * ds]);
	} else {
		const T akp1k = (T) 1 / s;
		const T ak = akp1k * d[i * ds], akp1 = akp1k * d[(i + 1) * ds];
		const T denom = (T) 1 / (ak * akp1 - (T) 1);
		const T xk = x[0] * akp1k, xkp1 = x[rs] * akp1k;
		x[0] = (akp1 * xk - xkp1) * denom;
		x[rs] = (ak * xkp1 - xk) * denom;
	}
}

// X <- L_unit B, n x n column major (reconstruct.rs:35-60)
template <typename T>
__global__ void lblt_scale_kernel(T *X, idx_t n, const T *L, idx_t rs, idx_t cs, const T *d, idx_t ds, const T *sub, idx_t ss)
{
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
	if (i >= n || j >= n)
		return;
	auto lu = [&](idx_t r, idx_t c) -> T { return r > c ? L[r * rs + c * cs] : (r == c ? (T) 1 : (T) 0); };
	T v = lu(i, j) * d[j * ds];
	const T s = sub[j * ss];
	if (s != (T) 0 && j + 1 < n)
		v += lu(i, j + 1) * s;
	else if (j > 0 && sub[(j - 1) * ss] != (T) 0)
		v += lu(i, j - 1) * sub[(j - 1) * ss];
	X[i + j * n] = v;
}

const char *strategy_name(int p)
{
	switch (p) {
	case FaerPivotingStrategy_Partial: return "Partial";
	case FaerPivotingStrategy_PartialDiag: return "PartialDiag";
	case FaerPivotingStrategy_Rook: return "Rook";
	case FaerPivotingStrategy_RookDiag: return "RookDiag";
	case FaerPivotingStrategy_Full: return "Full";
	}
	return "?";
}

template <typename T, typename I>
FaerLbltStatus factor_api(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut pf, FaerSliceMut pb, FaerLbltParams params)
{
	const idx_t n = (idx_t) A.nrows;
	FH_CHECK(A.nrows == A.ncols, "lblt: matrix must be square");
	FH_CHECK((idx_t) subdiag.len == n, "lblt: subdiag must have dim entries");
	const int p = (int) params.pivoting;
	if (!faer_hip_lblt_pivoting_supported(params.pivoting)) {
		fprintf(stderr, "faer_hip: fatal: lblt_factor_in_place: pivoting strategy %s (%d) is not one of Partial, PartialDiag, Rook, RookDiag, Full\n",
			strategy_name(p), p);
		fflush(stderr);
		abort();
	}
	const bool rook = p == FaerPivotingStrategy_Rook || p == FaerPivotingStrategy_RookDiag;
	const bool diagonal = p == FaerPivotingStrategy_PartialDiag || p == FaerPivotingStrategy_RookDiag;
	std::vector<idx_t> perm((size_t) n), perm_inv((size_t) n);
	long nt;
	{
		Staged<T> a(view<T>(A), true, true);
		Staged<T> sd(vview<T>(subdiag), false, true);
		nt = lblt_dev<T>(a.dev, sd.dev.p, sd.dev.rs, perm.data(), perm_inv.data(), rook, diagonal, p == FaerPivotingStrategy_Full);
	}
	store_perm<I>("lblt", pf, pb, perm.data(), perm_inv.data(), n);
	FaerLbltStatus stt;
	memset(&stt, 0, sizeof(stt));
	stt.tag = FaerLbltStatus_Ok;
	stt.ok.transposition_count = (size_t) nt;
	return stt;
}

// solve.rs:35-104
template <typename T> void solve_dev(MatV<const T> L, MatV<const T> d, MatV<const T> sd, const DevPerm &pf, const DevPerm &pb, MatV<T> X)
{
	const idx_t n = L.nrows, k = X.ncols;
	if (n == 0 || k == 0)
		return;
	permute_rows<T>(X, pf);
	trsm_lower_dev<T>(L, true, X);
	hipLaunchKernelGGL(lblt_block_diag_solve_kernel<T>, dim3((unsigned) ((n + 255) / 256), (unsigned) k), dim3(256), 0, ctx().stream, X.p, X.rs,
			   X.cs, n, k, d.p, d.rs, sd.p, sd.rs);
	FH_HIP(hipGetLastError());
	trsm_upper_dev<T>(L.t(), true, X);
	permute_rows<T>(X, pb);
}

template <typename T, typename I>
void solve_api(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs)
{
	const size_t n = L.nrows;
	FH_CHECK(L.ncols == n && rhs.nrows == n && diag.len == n && subdiag.len == n, "lblt solve: dimension mismatch");
	FH_CHECK(rhs.ncols < 65536, "lblt solve: too many right-hand sides");
	DevPerm fwd("lblt solve", pf, (idx_t) n, I{}), bwd("lblt solve", pb, (idx_t) n, I{});
	Staged<const T> l(view<T>(L), true, false), d(vview<T>(diag), true, false), sd(vview<T>(subdiag), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	solve_dev<T>(l.dev, d.dev, sd.dev, fwd, bwd, x.dev);
}

// reconstruct.rs:12-87 (the lower triangle of out only)
template <typename T, typename I>
void reconstruct_api(FaerMatMut Out, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef pf, FaerSliceRef pb)
{
	const idx_t n = (idx_t) L.nrows;
	FH_CHECK((idx_t) L.ncols == n && (idx_t) Out.nrows == n && (idx_t) Out.ncols == n && (idx_t) diag.len == n && (idx_t) subdiag.len == n,
		 "lblt reconstruct: dimension mismatch");
	FH_CHECK(n < 65536, "lblt reconstruct: dimension too large");
	check_perm_slice("lblt reconstruct", pf, n);
	DevPerm bwd("lblt reconstruct", pb, n, I{});
	if (n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), d(vview<T>(diag), true, false), sd(vview<T>(subdiag), true, false);
	Staged<T> o(view<T>(Out), true, true); // the strict upper triangle is kept
	Scratch xb((size_t) n * (size_t) n * sizeof(T) + 256), tb((size_t) n * (size_t) n * sizeof(T) + 256);
	MatV<T> X{xb.as<T>(), n, n, 1, n}, tmp{tb.as<T>(), n, n, 1, n};
	const dim3 grid((unsigned) ((n + 255) / 256), (unsigned) n);
	hipLaunchKernelGGL(lblt_scale_kernel<T>, grid, dim3(256), 0, ctx().stream, X.p, n, l.dev.p, l.dev.rs, l.dev.cs, d.dev.p, d.dev.rs, sd.dev.p,
			   sd.dev.rs);
	FH_HIP(hipGetLastError());
	matmul_triangular_dev<T>(tmp, (int) FaerBlock_TriangularLower, false, l.dev, (int) FaerBlock_UnitTriangularLower, X.t().c(),
				 (int) FaerBlock_Rectangular, (T) 1);
	sym_gather<T>(o.dev, tmp.p, bwd);
	ctx().sync();
}

// inverse.rs:11-42: solve with the identity
template <typename T, typename I>
void inverse_api(FaerMatMut Out, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef pf, FaerSliceRef pb)
{
	const size_t n = L.nrows;
	FH_CHECK(L.ncols == n && Out.nrows == n && Out.ncols == n && diag.len == n && subdiag.len == n, "lblt inverse: dimension mismatch");
	FH_CHECK(n < 65536, "lblt inverse: dimension too large");
	DevPerm fwd("lblt inverse", pf, (idx_t) n, I{}), bwd("lblt inverse", pb, (idx_t) n, I{});
	if (n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false), d(vview<T>(diag), true, false), sd(vview<T>(subdiag), true, false);
	Staged<T> o(view<T>(Out), false, true);
	svd_identity_dev<T>(o.dev);
	solve_dev<T>(l.dev, d.dev, sd.dev, fwd, bwd, o.dev);
}

size_t up64(size_t b) { return (b + 63) / 64 * 64; }

} // namespace

extern "C" {

void faer_hip_debug_lblt_last(size_t out[4])
{
	for (int i = 0; i < 4; ++i)
		out[i] = g_last[i];
}

#define X(suf, T)                                                                                                                                  \
	FaerLbltParams libfaer_v0_23_LbltParams_##suf(void) { return FaerLbltParams{FaerPivotingStrategy_PartialDiag, 128 * 128, 64}; }
X(f64, double)
X(f32, float)
#undef X

#define X(it, I, suf, T)                                                                                                                           \
	FaerLayout libfaer_v0_23_lblt_factor_in_place_scratch_##it##_##suf(size_t dim, FaerPar par, FaerLbltParams params)                         \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		size_t bs = params.block_size; /* factor.rs:1128-1140 */                                                                           \
		if (bs < 2 || dim <= bs)                                                                                                           \
			bs = 0;                                                                                                                    \
		return layout(dim == 0 ? 0 : up64(dim * sizeof(size_t)) + dim * bs * sizeof(T), 64);                                                 \
	}                                                                                                                                          \
	FaerLbltStatus libfaer_v0_23_lblt_factor_in_place_##it##_##suf(FaerMatMut A, FaerVecMut subdiag, FaerSliceMut perm_fwd,                    \
								       FaerSliceMut perm_bwd, FaerPar par, FaerMemAlloc mem, FaerLbltParams params) \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		return factor_api<T, I>(A, subdiag, perm_fwd, perm_bwd, params);                                                                   \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_lblt_solve_in_place_scratch_##it##_##suf(size_t dim, size_t rhs_ncols, FaerPar par)                               \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * rhs_ncols * sizeof(T), 64); /* solve.rs:11-18 */                                                                  \
	}                                                                                                                                          \
	void libfaer_v0_23_lblt_solve_in_place_##it##_##suf(FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerConj A_conj,                    \
							    FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerMatMut rhs, FaerPar par,             \
							    FaerMemAlloc mem)                                                                      \
	{                                                                                                                                          \
		(void) A_conj;                                                                                                                     \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		solve_api<T, I>(L, diag, subdiag, perm_fwd, perm_bwd, rhs);                                                                        \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_lblt_reconstruct_scratch_##it##_##suf(size_t dim, FaerPar par)                                                    \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * dim * sizeof(T), 64); /* reconstruct.rs:4-10 */                                                                   \
	}                                                                                                                                          \
	void libfaer_v0_23_lblt_reconstruct_##it##_##suf(FaerMatMut A, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd,   \
							 FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem)                                     \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		reconstruct_api<T, I>(A, L, diag, subdiag, perm_fwd, perm_bwd);                                                                    \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_lblt_inverse_scratch_##it##_##suf(size_t dim, FaerPar par)                                                        \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * dim * sizeof(T), 64); /* inverse.rs:3-9 */                                                                        \
	}                                                                                                                                          \
	void libfaer_v0_23_lblt_inverse_##it##_##suf(FaerMatMut A_inv, FaerMatRef L, FaerVecRef diag, FaerVecRef subdiag, FaerSliceRef perm_fwd,   \
						     FaerSliceRef perm_bwd, FaerPar par, FaerMemAlloc mem)                                         \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		inverse_api<T, I>(A_inv, L, diag, subdiag, perm_fwd, perm_bwd);                                                                    \
	}
X(u32, uint32_t, f64, double)
X(u64, uint64_t, f64, double)
X(u32, uint32_t, f32, float)
X(u64, uint64_t, f32, float)
#undef X

} // extern "C"
