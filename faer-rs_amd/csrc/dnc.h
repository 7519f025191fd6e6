// What the two divide and conquer drivers (evd.hip: symmetric tridiagonal, svd.hip: bidiagonal) share around their merges:
// the bit-pattern traits of the max-magnitude reductions, the input / output kernels (copy, the two power-of-two scalings,
// diag / offdiag, S), the host plan of the recursion with its device table, the forward rotation chain of the leaf kernels and
// the small host helpers (launch counts, leaf-size clamp, scratch carving, status read-back).  The merge kernels, the
// work vectors and the merge products stay with their solver; the scalar helpers and the root finder are in secular.h.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "secular.h"

namespace fh {

namespace {

// the bits of a non-negative float order like unsigned integers: atomicMax on them is a max of magnitudes
template <typename T> struct FloatBits;
template <> struct FloatBits<double> {
	typedef unsigned long long U;
	static __device__ U of(double x) { return (U) __double_as_longlong(x); }
	static __device__ double val(U u) { return __longlong_as_double((long long) u); }
	static constexpr double rmin = 1.0010415475915505e-146, rmax = 9.989595361011175e+145; // sqrt(sml / eps), 1 / rmin
};
template <> struct FloatBits<float> {
	typedef unsigned int U;
	static __device__ U of(float x) { return __float_as_uint(x); }
	static __device__ float val(U u) { return __uint_as_float(u); }
	static constexpr float rmin = 3.1401849e-16f, rmax = 3.1845258e+15f;
};

// ---- input / output kernels ---------------------------------------------------------------------
enum DncTriangle { DNC_ALL = 0, DNC_LOWER = 1, DNC_UPPER = 2 };

// X (m x n, dense column major) <- the `tri` part of A, zero elsewhere: the rest of A is never read.  Also max |X|: one
// atomic per block.
template <typename T>
__global__ __launch_bounds__(256) void dnc_copy_kernel(const T *A, idx_t rs, idx_t cs, T *X, idx_t m, idx_t n, int tri,
							typename FloatBits<T>::U *amax)
{
	__shared__ T red[4];
	const idx_t t = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	T v = 0;
	if (t < m * n) {
		const idx_t i = t % m, j = t / m;
		const bool keep = tri == DNC_ALL || (tri == DNC_LOWER ? i >= j : i <= j);
		v = keep ? A[i * rs + j * cs] : (T) 0;
		X[t] = v;
	}
	const T mx = block_reduce<T, true>(ev_abs(v), red);
	if (threadIdx.x == 0)
		atomicMax(amax, FloatBits<T>::of(mx));
}

// the scaling of LAPACK's xSYEV: a matrix whose largest entry lies outside [rmin, rmax] is scaled by a power of two into that
// range (exact), the eigenvalues / singular values are scaled back at the end; fac[0] <- the factor (1 inside the range)
template <typename T> __global__ void dnc_scale_kernel(T *X, idx_t nn, const typename FloatBits<T>::U *amax, T *fac)
{
	const T a = FloatBits<T>::val(*amax);
	int e = 0;
	if (isfinite(a) && a > (T) 0) {
		if (a > FloatBits<T>::rmax)
			e = ilogb((double) FloatBits<T>::rmax) - ilogb((double) a) - 1;
		else if (a < FloatBits<T>::rmin)
			e = ilogb((double) FloatBits<T>::rmin) - ilogb((double) a) + 1;
	}
	if (e == 0) {
		if (blockIdx.x == 0 && threadIdx.x == 0)
			fac[0] = 1;
		return;
	}
	const T f = (T) ldexp(1.0, e);
	const idx_t t = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (t < nn)
		X[t] *= f;
	if (t == 0)
		fac[0] = f;
}

// diag / offdiag of the condensed form in X (leading dimension ldx; the off-diagonal entry sits `step` elements behind the
// diagonal one: 1 for the tridiagonal, ldx for the upper bidiagonal) and max(|d|, |e|); any non-finite entry sets the status
// before any iteration
template <typename T>
__global__ __launch_bounds__(256) void dnc_extract_kernel(const T *X, idx_t ldx, idx_t step, idx_t n, T *D, T *E,
							   typename FloatBits<T>::U *tmax, int *status)
{
	__shared__ T red[4];
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	T m = 0;
	if (i < n) {
		const T d = X[i + i * ldx];
		const T e = i + 1 < n ? X[i + i * ldx + step] : (T) 0;
		D[i] = d;
		E[i] = e;
		if (!isfinite(d) || !isfinite(e))
			status[0] = 1;
		m = ev_max(ev_abs(d), ev_abs(e));
	}
	m = block_reduce<T, true>(m, red);
	if (threadIdx.x == 0)
		atomicMax(tmax, FloatBits<T>::of(m));
}

// The root finder's stopping tests compare secular-function values with eps in absolute terms (bidiag_svd.rs:64-66), so
// the solve is not scale invariant: d / e are scaled by a power of two (exact) to max(|d|, |e|) in [1, 2).
// tfac[0] <- the factor.
template <typename T> __global__ void dnc_tscale_kernel(T *D, T *E, idx_t n, const typename FloatBits<T>::U *tmax, T *tfac)
{
	const T a = FloatBits<T>::val(*tmax);
	const int e = isfinite(a) && a > (T) 0 ? -ilogb((double) a) : 0;
	const T f = (T) ldexp(1.0, e);
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) {
		D[i] *= f;
		E[i] *= f;
	}
	if (i == 0)
		tfac[0] = f;
}

template <typename T> __global__ void dnc_write_s_kernel(const T *D, idx_t n, T *S, idx_t ss, const T *fac) // fac: the two scale factors
{
	const idx_t i = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
		S[i * ss] = D[i] * ((T) 1 / fac[0]) * ((T) 1 / fac[1]);
}

// ---- the rotation chain of the leaf kernels -----------------------------------------------------
// A sweep's rotations (rc[k], rsn[k]) applied to one row: rotations on the right act on each row on its own, so every lane
// walks the whole chain for its rows.  apply_on_the_right_in_place on columns (k + 1, k), k = first .. last - 1:
// X(:, k+1) = c a + s b, X(:, k) = c b - s a
template <typename T> __device__ __forceinline__ void rot_chain_forward(T *row, int first, int last, const T *rc, const T *rsn)
{
	T x = row[first];
	for (int k = first; k < last; ++k) {
		const T a = row[k + 1], c = rc[k], s = rsn[k];
		row[k] = c * x - s * a;
		x = c * a + s * x;
	}
	row[last] = x;
}

// ---- host: the plan of the recursion ------------------------------------------------------------
struct DncNode {
	idx_t off, n;
	int depth;
};

// A node of more than `leaf` entries splits at k = n / 2 into [off, off + k) and [off + k + gap, off + n): gap = 0 for the
// tridiagonal problem, 1 for the bidiagonal one (entry k is the merge's own row).
inline void dnc_plan(idx_t off, idx_t n, int depth, idx_t leaf, idx_t gap, std::vector<DncNode> &leaves, std::vector<std::vector<DncNode>> &merges)
{
	if (n <= leaf) {
		leaves.push_back(DncNode{off, n, depth});
		return;
	}
	if ((int) merges.size() <= depth)
		merges.resize((size_t) depth + 1);
	merges[(size_t) depth].push_back(DncNode{off, n, depth});
	const idx_t k = n / 2;
	dnc_plan(off, k, depth + 1, leaf, gap, leaves, merges);
	dnc_plan(off + k + gap, n - k - gap, depth + 1, leaf, gap, leaves, merges);
}

// The tree follows from n and the leaf size alone, so the host plans it once.  tab: three ints per leaf (offset, size, depth
// parity), then level by level three ints per merge (offset, size, size / 2); level_at[lv]: where level lv starts in tab.
struct DncPlan {
	std::vector<DncNode> leaves;
	std::vector<std::vector<DncNode>> merges; // by depth
	std::vector<int> tab;
	std::vector<size_t> level_at;
	std::vector<idx_t> maxn; // the largest merge of every level
	size_t nmerges = 0, max_level = 0;

	DncPlan(idx_t n, idx_t leaf, idx_t gap, const char *too_many)
	{
		dnc_plan(0, n, 0, leaf, gap, leaves, merges);
		for (const DncNode &l : leaves) {
			tab.push_back((int) l.off);
			tab.push_back((int) l.n);
			tab.push_back(l.depth & 1);
		}
		for (const std::vector<DncNode> &ms : merges) {
			level_at.push_back(tab.size());
			nmerges += ms.size();
			max_level = std::max(max_level, ms.size());
			idx_t mx = 0;
			for (const DncNode &m : ms) {
				tab.push_back((int) m.off);
				tab.push_back((int) m.n);
				tab.push_back((int) (m.n / 2));
				mx = std::max(mx, m.n);
			}
			maxn.push_back(mx);
		}
		FH_CHECK(leaves.size() < (1u << 31) && max_level < 65536, too_many);
	}
	int levels() const { return (int) merges.size(); }
	size_t tab_bytes() const { return tab.size() * sizeof(int); }
	// the plan must outlive the copy: the drivers synchronize the stream before they return
	void upload(int *tab_dev, hipStream_t s) const { FH_HIP(hipMemcpyAsync(tab_dev, tab.data(), tab_bytes(), hipMemcpyHostToDevice, s)); }
};

// ---- host: small helpers ------------------------------------------------------------------------
inline unsigned blocks_for(idx_t count, int per) { return (unsigned) ((count + per - 1) / per); }

// leaves of min(max(recursion_threshold, 4), cap) entries
inline idx_t dnc_leaf_size(size_t recursion_threshold, size_t cap) { return (idx_t) std::min(std::max(recursion_threshold, (size_t) 4), cap); }

// hands out n entries from p to each of dst in turn
template <typename P> inline void dnc_carve(P *&p, idx_t n, std::initializer_list<P **> dst)
{
	for (P **q : dst) {
		*q = p;
		p += n;
	}
}

// the one host synchronization of a call: status[0] through the pinned word
inline int dnc_read_status(const int *status, hipStream_t s)
{
	int *st = ctx().pinned_ints();
	FH_HIP(hipMemcpyAsync(st, status, sizeof(int), hipMemcpyDeviceToHost, s));
	FH_HIP(hipStreamSynchronize(s));
	return st[0];
}

} // namespace

} // namespace fh
