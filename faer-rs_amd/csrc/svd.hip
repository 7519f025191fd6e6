// Singular value decomposition -- faer/src/linalg/svd/mod.rs:326-431, :530-671 (svd) with the divide and conquer solver of
// the bidiagonal problem, svd/bidiag_svd.rs:1005-1490 (divide_and_conquer, the MatU::Full arm) and :274-476 (qr_algorithm),
// on the device.
//
//   [n > m: transposed view, U and V swapped]  [m / n > qr_ratio_threshold: geqrf_dev, continue with R]
//   copy -> bidiag_dev (condense.hip) -> diag / superdiag -> bidiagonal solve -> two block Householder back-transforms
//   (apply_householder_sequence_left_dev) -> S.
//
// The bidiagonal solve follows the reference's recursion on the transposed (n + 1) x n lower bidiagonal problem (split at
// k = n / 2, rem = n - k - 1; the superdiagonal plays `subdiag`), so the (n + 1) x (n + 1) factor P becomes V and the n x n
// factor Q becomes U (mod.rs:393-415).  A node at offset `off` owns P[off .. off + n], Q[off .. off + n) as diagonal blocks
// of two (N + 1)^2 / N^2 buffers; children and parents alternate between two buffers by depth parity.  It runs level by
// level, bottom up; every launch covers all nodes of one level:
//   * svd_leaf_kernel: one single-wave workgroup per leaf of at most min(max(recursion_threshold, 4), L) entries, L = 64
//     for fp64 and fp32 (svd_leaf_size), both factors in LDS ((L + 1) x 65 + L x 65 elements: 65.5 KiB fp64, 32.8 KiB fp32
//     of the 160 KiB; the budget alone would allow L = 96 for fp64, but lane 0's rotation chain grows as the square of the
//     leaf size, which is why evd.hip stopped at 64 as well).  The Givens sweep that removes the extra row (:1029-1044), then
//     the zero-shift chase / shifted QR sweeps with the reference's iteration cap: lane 0 generates a sweep's rotations,
//     every lane applies them to its rows of P and Q.
//   * svd_merge_prep_kernel (one workgroup per merge): the node's scale, alpha, beta, lambda, phi, r0, c0, s0, col0 and the
//     shifted diag (:1171-1251), deflate with deflation_43 / deflation_44 and the permutation (:794-965; the transposition
//     bookkeeping is replaced by the order it produces), the compacted secular problem.
//   * svd_secular_kernel (one wavefront per root): secular_root of secular.h on 1 + sum c_i^2 / ((d_i - s)(d_i + s)), then a
//     sign check of the root with a bisection where the reference's absolute stopping test left it short of the pole.
//   * svd_zhat_kernel (one thread per entry): perturb_col0 (:655-706) and the final (nonincreasing) column order.
//   * svd_vectors_kernel (one workgroup per column): compute_singular_vectors (:592-654), then the recorded deflation
//     rotations on the column (:1297-1327; rows of one column form a chain, columns are independent), then the column is
//     written in the children's row order with the rank-one terms of :1415-1441 folded in (row 0 of M feeds row k of the
//     first child with c0 and the last row of the second with s0; the last column is (-s0 q1, c0 q2)).
//   * merge products on gemm_dev: two for P, two plus one copied row for Q (:1330-1445).
// The shapes of every launch follow from n and the leaf size alone (deflation changes contents only: deflated columns are
// unit vectors), so the solve has no host synchronization; the call reads back one status word at its end.
// Values only: the P recursion runs into scratch (col0 of every merge needs rows of P) and is discarded; Q and the two
// back-transforms are skipped.  With V only, Q is skipped as well; with U only, P is still needed for col0.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "dnc.h"

namespace fh {

namespace {

constexpr int SVD_LEAF_MAX = 64;

// per-level work vectors (a merge at offset `off` owns [off, off + n)); per-merge scalars by the merge's index in its level
template <typename T> struct SvdWork {
	T *dt, *ct;	     // diag / col0 of M in the children's order
	T *dg, *c0;	     // after deflation, in sorted positions
	T *dp, *zp;	     // the non-deflated entries, compacted (diag_perm, col0_perm)
	T *sh, *mu, *sv, *zh; // roots as (shift, mu), singular values of M, z-hat
	T *jc, *js;	     // recorded rotations: [0, n0i) of deflation_43, [n0i, n0i + nij) of deflation_44
	int *op, *pm, *nxt, *jidx, *colpos, *tmp;
	T *sc;	  // 4 per merge: c0, s0, max, |col0|
	int *cnt; // 8 per merge: zero node, m (non-deflated), actual_n by col0, n0i, nij
};

// ---- leaves -------------------------------------------------------------------------------------
constexpr int svd_leaf_ld(int m) { return (m + 1) | 1; }
template <typename T> constexpr size_t svd_leaf_lds(int m)
{
	return ((size_t) (2 * m + 1) * svd_leaf_ld(m) + 6 * (SVD_LEAF_MAX + 1)) * sizeof(T) + (SVD_LEAF_MAX + 1) * sizeof(int);
}

// one wavefront per leaf; leaves[3 * b ..]: offset, entries, buffer (depth parity)
template <typename T>
__global__ __launch_bounds__(64) void svd_leaf_kernel(const int *leaves, const T *D0, const T *E0, T *D, T *P0, T *P1, idx_t ldp, T *Q0, T *Q1,
						      idx_t ldq, int want_q, int *status)
{
	extern __shared__ __align__(16) unsigned char svd_lds[];
	__shared__ int sh_ctl[4]; // start, end, flag
	const int tid = threadIdx.x;
	const idx_t off = leaves[3 * blockIdx.x];
	const int m = leaves[3 * blockIdx.x + 1];
	const int par = leaves[3 * blockIdx.x + 2];
	if (status[0])
		return;
	T *Pg = par ? P1 : P0, *Qg = par ? Q1 : Q0;
	const int ld = svd_leaf_ld(m);
	T *p = reinterpret_cast<T *>(svd_lds);	  // (m + 1) x (m + 1), row major
	T *q = p + (size_t) (m + 1) * ld;	  // m x m, row major
	T *d = q + (size_t) m * ld, *e = d + (SVD_LEAF_MAX + 1);
	T *c1 = e + (SVD_LEAF_MAX + 1), *s1 = c1 + (SVD_LEAF_MAX + 1), *c2 = s1 + (SVD_LEAF_MAX + 1), *s2 = c2 + (SVD_LEAF_MAX + 1);
	int *perm = reinterpret_cast<int *>(s2 + (SVD_LEAF_MAX + 1));
	const T eps = DncTraits<T>::eps, sml = DncTraits<T>::sml;

	for (int t = tid; t < (m + 1) * ld; t += 64)
		p[t] = (t % ld) == (t / ld) ? (T) 1 : (T) 0;
	for (int t = tid; t < m * ld; t += 64)
		q[t] = (t % ld) == (t / ld) ? (T) 1 : (T) 0;
	for (int i = tid; i < m; i += 64) {
		d[i] = D0[off + i];
		e[i] = E0[off + i];
		perm[i] = i;
	}
	__syncthreads();
	// the extra row (bidiag_svd.rs:1029-1044)
	if (tid == 0) {
		T val = e[m - 1];
		e[m - 1] = 0;
		for (int i = m - 1; i >= 0; --i) {
			T c, s;
			make_givens(d[i], val, c, s);
			d[i] = c * d[i] - s * val;
			if (i > 0) {
				val = s * e[i - 1];
				e[i - 1] = c * e[i - 1];
			}
			c1[i] = c;
			s1[i] = s;
		}
	}
	__syncthreads();
	for (int r = tid; r <= m; r += 64) {
		T *row = p + (size_t) r * ld;
		T y = row[m];
		for (int i = m - 1; i >= 0; --i) {
			const T x = row[i], c = c1[i], s = s1[i];
			row[i] = c * x - s * y;
			y = c * y + s * x;
		}
		row[m] = y;
	}
	__syncthreads();
	// qr_algorithm (:274-476)
	T mx = 0;
	for (int i = tid; i < m; i += 64)
		mx = ev_max(mx, ev_max(ev_abs(d[i]), ev_abs(e[i])));
	mx = wave_max(mx);
	mx = __shfl(mx, 0);
	bool fail = false;
	if (mx != (T) 0) {
		const T inv = (T) 1 / mx;
		for (int i = tid; i < m; i += 64) {
			d[i] *= inv;
			e[i] *= inv;
		}
		__syncthreads();
		const long max_iters = DncTraits<T>::iter_factor * (long) m * (long) m;
		const T eps2 = eps * eps;
		for (long iter = 0; iter < max_iters; ++iter) {
			for (int i = tid; i + 1 < m; i += 64)
				if (e[i] * e[i] <= eps2 * ev_abs(d[i] * d[i + 1]) + sml)
					e[i] = 0;
			__syncthreads();
			if (tid == 0) {
				int end = m;
				while (end >= 2 && e[end - 2] * e[end - 2] <= sml)
					--end;
				int start = end - 1;
				while (start >= 1 && e[start - 1] != (T) 0)
					--start;
				sh_ctl[0] = start;
				sh_ctl[1] = end;
			}
			__syncthreads();
			const int start = sh_ctl[0], end = sh_ctl[1];
			if (end <= 1)
				break;
			bool found_zero_diag = false;
			for (int i = start; i < end - 1; ++i) {
				if (!(ev_abs(d[i]) <= eps)) // the same LDS word for every lane
					continue;
				found_zero_diag = true;
				__syncthreads();
				if (tid == 0) {
					T val = e[i];
					e[i] = 0;
					for (int j = i + 1; j < end; ++j) {
						T c, s;
						make_givens(d[j], val, c, s);
						d[j] = c * d[j] - s * val;
						if (j + 1 < end) {
							val = s * e[j];
							e[j] = c * e[j];
						}
						c1[j] = c;
						s1[j] = s;
					}
				}
				__syncthreads();
				if (want_q)
					for (int r = tid; r < m; r += 64) {
						T *row = q + (size_t) r * ld;
						T y = row[i];
						for (int j = i + 1; j < end; ++j) {
							const T x = row[j], c = c1[j], s = s1[j];
							row[j] = c * x - s * y;
							y = c * y + s * x;
						}
						row[i] = y;
					}
				__syncthreads();
			}
			if (found_zero_diag) {
				if (iter + 1 == max_iters) {
					fail = true;
					break;
				}
				continue;
			}
			if (tid == 0) {
				const int end2 = end - 2, end1 = end - 1;
				const T t00 = end - start == 2 ? d[end2] * d[end2] : d[end2] * d[end2] + e[end - 3] * e[end - 3];
				const T t11 = d[end1] * d[end1] + e[end2] * e[end2];
				const T t01 = d[end2] * e[end2];
				const T t01_2 = t01 * t01;
				T mu;
				if (t01_2 > sml) {
					const T dd = (t00 - t11) * (T) 0.5;
					T delta = ev_sqrt(dd * dd + t01_2);
					if (dd < (T) 0)
						delta = -delta;
					mu = t11 - t01_2 / (dd + delta);
				} else {
					mu = t11;
				}
				T y = d[start] * d[start] - mu;
				T z = d[start] * e[start];
				for (int k = start; k < end1; ++k) {
					T c, s;
					make_givens(y, z, c, s);
					if (k > start)
						e[k - 1] = ev_abs(c * y - s * z);
					T dk = d[k];
					const T t0 = c * dk - s * e[k], t1 = s * dk + c * e[k];
					dk = t0;
					e[k] = t1;
					y = dk;
					z = -s * d[k + 1];
					d[k + 1] = c * d[k + 1];
					c1[k] = c;
					s1[k] = s;
					make_givens(y, z, c, s);
					dk = c * y - s * z;
					d[k] = dk;
					const T u0 = c * e[k] - s * d[k + 1], u1 = s * e[k] + c * d[k + 1];
					e[k] = u0;
					d[k + 1] = u1;
					if (k < end - 2) {
						y = e[k];
						z = -s * e[k + 1];
						e[k + 1] = c * e[k + 1];
					}
					c2[k] = c;
					s2[k] = s;
				}
			}
			__syncthreads();
			for (int r = tid; r <= m; r += 64)
				rot_chain_forward(p + (size_t) r * ld, start, end - 1, c1, s1);
			if (want_q)
				for (int r = tid; r < m; r += 64)
					rot_chain_forward(q + (size_t) r * ld, start, end - 1, c2, s2);
			__syncthreads();
			if (iter + 1 == max_iters) {
				fail = true;
				break;
			}
		}
		if (!fail) {
			__syncthreads();
			// signs (:436-446; c1 holds the sign of column j of Q) and the descending order (:447-468)
			for (int j = tid; j < m; j += 64) {
				const bool neg = d[j] < (T) 0;
				if (neg)
					d[j] = -d[j];
				c1[j] = neg ? (T) -1 : (T) 1;
			}
			__syncthreads();
			if (tid == 0) {
				for (int k = 0; k < m; ++k) {
					T best = 0;
					int idx = k;
					for (int kk = k; kk < m; ++kk)
						if (d[kk] > best) {
							best = d[kk];
							idx = kk;
						}
					if (idx != k) {
						const T a = d[k];
						d[k] = d[idx];
						d[idx] = a;
						const int t = perm[k];
						perm[k] = perm[idx];
						perm[idx] = t;
					}
				}
			}
			__syncthreads();
		}
	} else {
		for (int j = tid; j < m; j += 64)
			c1[j] = 1;
		__syncthreads();
	}
	if (fail) {
		if (tid == 0)
			status[0] = 1;
		return;
	}
	for (int i = tid; i < m; i += 64)
		D[off + i] = d[i] * mx;
	for (int t = tid; t < (m + 1) * (m + 1); t += 64) {
		const int i = t % (m + 1), j = t / (m + 1);
		Pg[(off + i) + (off + j) * ldp] = p[(size_t) i * ld + (j < m ? perm[j] : m)];
	}
	if (want_q)
		for (int t = tid; t < m * m; t += 64) {
			const int i = t % m, j = t / m;
			Qg[(off + i) + (off + j) * ldq] = q[(size_t) i * ld + perm[j]] * c1[perm[j]];
		}
}

// ---- merges ---------------------------------------------------------------------------------------
// merges[3 * b ..]: offset, entries n, k (the first child; the second has n - k - 1)
template <typename T>
__global__ __launch_bounds__(256) void svd_merge_prep_kernel(const int *merges, const T *D0, const T *E0, const T *D, const T *Pc, idx_t ldp,
							     SvdWork<T> w, const int *status)
{
	__shared__ T red[4];
	__shared__ int sh_n0i;
	if (status[0])
		return;
	const int b = blockIdx.x, tid = threadIdx.x;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1], k = merges[3 * b + 2];
	const T eps = DncTraits<T>::eps, sml = DncTraits<T>::sml;
	T *dt = w.dt + off, *ct = w.ct + off, *dg = w.dg + off, *c0 = w.c0 + off, *dp = w.dp + off, *zp = w.zp + off;
	T *jc = w.jc + off, *js = w.js + off;
	int *op = w.op + off, *pm = w.pm + off, *nxt = w.nxt + off, *jidx = w.jidx + off, *ord = w.tmp + off;
	// the node's scale (:1065-1089)
	T m0 = 0;
	for (int i = tid; i < n; i += 256)
		m0 = ev_max(m0, ev_max(ev_abs(D0[off + i]), ev_abs(E0[off + i])));
	const T mx = block_reduce<T, true>(m0, red);
	if (mx == (T) 0) {
		if (tid == 0) {
			w.cnt[8 * b] = 1;
			w.sc[4 * b + 2] = 0;
		}
		return;
	}
	const T inv = (T) 1 / mx;
	// :1171-1251
	const T alpha = D0[off + k] * inv, beta = E0[off + k] * inv;
	const T lambda = Pc[(off + k) + (off + k) * ldp], phi = Pc[(off + k + 1) + (off + n) * ldp];
	const T al = alpha * lambda, bp = beta * phi;
	const T r0 = ev_sqrt(al * al + bp * bp);
	const T cc0 = r0 == (T) 0 ? (T) 1 : al / r0, ss0 = r0 == (T) 0 ? (T) 0 : bp / r0;
	T md = 0, mc = 0;
	for (int j = tid; j < n; j += 256) {
		T dv, cv;
		if (j == 0) {
			dv = r0;
			cv = r0;
		} else if (j <= k) {
			dv = D[off + j - 1] * inv;
			cv = alpha * Pc[(off + k) + (off + j - 1) * ldp];
			md = ev_max(md, ev_abs(dv));
		} else {
			dv = D[off + j] * inv;
			cv = beta * Pc[(off + k + 1) + (off + j) * ldp];
			md = ev_max(md, ev_abs(dv));
		}
		dt[j] = dv;
		ct[j] = cv;
		mc = ev_max(mc, ev_abs(cv));
	}
	const T max_diag = block_reduce<T, true>(md, red);
	const T max_col0 = block_reduce<T, true>(mc, red);
	// deflate (:794-923)
	const T eps_strict = ev_max(eps * max_diag, sml);
	const T eps_coarse = (T) 8 * eps * ev_max(max_diag, max_col0);
	__syncthreads();
	if (tid == 0 && dt[0] < eps_coarse) {
		dt[0] = eps_coarse;
		ct[0] = eps_coarse;
	}
	for (int i = tid; i < n; i += 256)
		if (i >= 1 && ev_abs(ct[i]) < eps_strict)
			ct[i] = 0;
	__syncthreads();
	if (tid == 0) {
		// deflation_43: a chain through col0[0]
		int n0i = 0;
		T p0 = ct[0];
		for (int i = 1; i < n; ++i) {
			if (!(dt[i] < eps_coarse))
				continue;
			const T qv = ct[i];
			if (p0 == (T) 0 && qv == (T) 0)
				continue;
			T c, s;
			make_givens(p0, qv, c, s);
			p0 = c * p0 - s * qv;
			ct[i] = 0;
			jc[n0i] = c;
			js[n0i] = s;
			jidx[n0i] = i;
			++n0i;
		}
		ct[0] = p0;
		dt[0] = p0;
		sh_n0i = n0i;
	}
	__syncthreads();
	int some = 0;
	for (int i = tid; i < n; i += 256)
		if (i >= 1 && !(ev_abs(ct[i]) < sml))
			some = 1;
	const bool total = !__syncthreads_or(some);
	if (tid == 0) {
		// the merge of the two descending halves without the entries below sml (:842-866), then the positions: 0 first, the
		// rest ascending, the entries below sml last (what the transpositions of :879-898 produce)
		int i = 1, j = k + 1, nd = 0;
		while (i <= k || j < n) {
			int pick;
			if (i > k)
				pick = j++;
			else if (j >= n)
				pick = i++;
			else if (dt[i] < dt[j])
				pick = j++;
			else
				pick = i++;
			if (!(ev_abs(dt[pick]) < sml))
				ord[nd++] = pick;
		}
		int pos = 0;
		if (!total) {
			op[pos++] = 0;
			for (int t = nd - 1; t >= 0; --t)
				op[pos++] = ord[t];
		} else {
			// total deflation: entry 0 takes its place among the others (:867-878)
			bool placed = false;
			for (int t = nd - 1; t >= 0; --t) {
				if (!placed && dt[ord[t]] > dt[0]) {
					op[pos++] = 0;
					placed = true;
				}
				op[pos++] = ord[t];
			}
			if (!placed)
				op[pos++] = 0;
		}
		for (int t = n - 1; t >= 1; --t)
			if (ev_abs(dt[t]) < sml)
				op[pos++] = t;
	}
	__syncthreads();
	for (int i = tid; i < n; i += 256) {
		const int src = op[i];
		dg[i] = dt[src];
		c0[i] = i == 0 ? dt[src] : (total ? (T) 0 : ct[src]);
	}
	__syncthreads();
	if (tid == 0) {
		const int n0i = sh_n0i;
		int nij = 0;
		// deflation_44 (:906-921)
		int i = n - 1;
		while (i > 0 && (ev_abs(dg[i]) < sml || ev_abs(c0[i]) < sml))
			--i;
		while (i > 1) {
			if (dg[i] - dg[i - 1] < eps_strict) {
				const T pv = c0[i - 1], qv = c0[i];
				if (!(pv == (T) 0 && qv == (T) 0)) {
					T c, s;
					make_givens(pv, qv, c, s);
					c0[i - 1] = c * pv - s * qv;
					c0[i] = 0;
					jc[n0i + nij] = c;
					js[n0i + nij] = s;
					jidx[n0i + nij] = i;
					++nij;
				}
				dg[i - 1] = dg[i];
			}
			--i;
		}
		// compute_svd_of_m :489-520, compute_singular_values :717-720
		dg[0] = 0;
		int an_d = n;
		while (an_d > 1 && dg[an_d - 1] == (T) 0)
			--an_d;
		int m = 0;
		T ss = 0;
		for (int t = 0; t < n; ++t) {
			const T cv = c0[t];
			ss += cv * cv;
			if (t < an_d && cv != (T) 0) {
				pm[m] = t;
				dp[m] = dg[t];
				zp[m] = cv;
				++m;
			}
		}
		int an_c = n;
		while (an_c > 1 && c0[an_c - 1] == (T) 0)
			--an_c;
		int nx = -1;
		for (int t = n - 1; t >= 0; --t) {
			nxt[t] = nx;
			if (c0[t] != (T) 0)
				nx = t;
		}
		w.cnt[8 * b] = 0;
		w.cnt[8 * b + 1] = m;
		w.cnt[8 * b + 2] = an_c;
		w.cnt[8 * b + 3] = n0i;
		w.cnt[8 * b + 4] = nij;
		w.sc[4 * b] = cc0;
		w.sc[4 * b + 1] = ss0;
		w.sc[4 * b + 2] = mx;
		w.sc[4 * b + 3] = ev_sqrt(ss);
	}
}

// secular_eq (:760-774) evaluated by a whole wavefront; every lane holds the same scalars
template <typename T> struct SvdSecularEq {
	const T *d, *z;
	int m;
	__device__ T operator()(T shift, T mu) const
	{
		T acc = 0;
		for (int i = (int) (threadIdx.x & 63); i < m; i += 64) {
			const T c = z[i], di = d[i];
			acc += (c / ((di - shift) - mu)) * (c / ((di + shift) + mu));
		}
		return (T) 1 + wave_sum(acc);
	}
};

// compute_singular_values (:707-759): one wavefront per root; grid (ceil(max n / 4), merges)
template <typename T> __global__ __launch_bounds__(256) void svd_secular_kernel(const int *merges, SvdWork<T> w, const int *status)
{
	if (status[0])
		return;
	const int b = blockIdx.y;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1];
	const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n || w.cnt[8 * b])
		return;
	const int m = w.cnt[8 * b + 1], an_c = w.cnt[8 * b + 2];
	const T *dg = w.dg + off, *c0 = w.c0 + off;
	if (c0[i] == (T) 0 || an_c == 1) {
		if ((threadIdx.x & 63) == 0) {
			const T s = i == 0 ? c0[0] : dg[i];
			w.sv[off + i] = s;
			w.sh[off + i] = s;
			w.mu[off + i] = 0;
		}
		return;
	}
	const bool last = i == an_c - 1;
	const T left = dg[i];
	const T right = last ? dg[an_c - 1] + w.sc[4 * b + 3] : dg[w.nxt[off + i]];
	SvdSecularEq<T> f{w.dp + off, w.zp + off, m};
	T shift, mu;
	secular_root<T>(f, left, right, last, shift, mu);
	// The reference's secant iteration stops once the function changes by less than eps between two iterates (an absolute
	// test).  With a col0 entry just above the deflation threshold the root lies within ~z^2 of its pole while the function is
	// flat to working precision over the rest of the bracket, so the iteration stops orders of magnitude away from the root:
	// the singular value is still accurate, but z-hat, which takes (sigma - pole) as a factor, is not (residuals of
	// 9 N eps ||A|| in fp32, where such entries are common).  f increases with mu on (0, right - left) for the left pole and on
	// (left - right, 0) for the right one: a root that does not separate the signs of f at mu (1 -+ 16 eps) is bisected.
	{
		const T eps = DncTraits<T>::eps, tol = (T) 16 * eps;
		const T a = mu * ((T) 1 - tol), b = mu * ((T) 1 + tol);
		const T lo = a < b ? a : b, hi = a < b ? b : a;
		const T flo = f(shift, lo), fhi = f(shift, hi);
		if (!(flo <= (T) 0 && fhi >= (T) 0)) {
			T blo = shift == left ? (T) 0 : left - right, bhi = shift == left ? right - left : (T) 0;
			if (flo > (T) 0)
				bhi = lo;
			else
				blo = hi;
			for (int it = 0; it < 2200 && bhi - blo > (T) 2 * eps * ev_max(ev_abs(blo), ev_abs(bhi)); ++it) {
				T mid = (blo + bhi) * (T) 0.5;
				if (blo != (T) 0 && bhi != (T) 0) { // same sign: the geometric mean closes in on a root next to the pole faster
					T g = ev_sqrt(ev_abs(blo)) * ev_sqrt(ev_abs(bhi));
					if (blo < (T) 0)
						g = -g;
					if (blo < g && g < bhi)
						mid = g;
				}
				const T fm = f(shift, mid);
				if (fm == (T) 0) {
					blo = mid;
					bhi = mid;
				} else if (fm > (T) 0) {
					bhi = mid;
				} else {
					blo = mid;
				}
			}
			mu = (blo + bhi) * (T) 0.5;
		}
	}
	if ((threadIdx.x & 63) == 0) {
		w.sv[off + i] = shift + mu;
		w.sh[off + i] = shift;
		w.mu[off + i] = mu;
	}
}

// perturb_col0 (:655-706) and the column of every singular value of M in the nonincreasing order; the merged values go to D.
// grid (ceil(max n / 256), merges)
template <typename T> __global__ __launch_bounds__(256) void svd_zhat_kernel(const int *merges, SvdWork<T> w, T *D, const int *status)
{
	if (status[0])
		return;
	const int b = blockIdx.y;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1];
	const int kk = blockIdx.x * 256 + threadIdx.x;
	if (kk >= n)
		return;
	if (w.cnt[8 * b]) {
		D[off + kk] = 0;
		w.colpos[off + kk] = kk;
		return;
	}
	const int m = w.cnt[8 * b + 1];
	const T *dg = w.dg + off, *c0 = w.c0 + off, *sv = w.sv + off, *sh = w.sh + off, *mu = w.mu + off;
	const int *pm = w.pm + off;
	T zh = 0;
	if (m > 0 && c0[kk] != (T) 0) {
		const int li = pm[m - 1];
		const T dk = dg[kk];
		T prod = (sv[li] + dk) * (mu[li] + (sh[li] - dk));
		for (int l = 0; l < m; ++l) {
			const int i = pm[l];
			if (i == kk)
				continue;
			if (i >= kk && l == 0) {
				prod = 0;
				break;
			}
			const int j = i < kk ? i : (l > 0 ? pm[l - 1] : i);
			prod *= ((sv[j] + dk) / (dg[i] + dk)) * ((mu[j] + (sh[j] - dk)) / (dg[i] - dk));
		}
		const T t = ev_sqrt(prod);
		zh = c0[kk] > (T) 0 ? t : -t;
	}
	w.zh[off + kk] = zh;
	// nonincreasing; equal values in descending position, as the reversal of :582-585 leaves them
	const T s = sv[kk];
	int rank = 0;
	for (int t = 0; t < n; ++t) {
		const T st = sv[t];
		rank += (st > s) || (st == s && t > kk);
	}
	w.colpos[off + kk] = rank;
	D[off + rank] = s * w.sc[4 * b + 2];
}

// compute_singular_vectors (:592-654), the recorded rotations (:1297-1327) and the rows in the children's order; grid
// (max n, merges), one column of M's factors per workgroup.  Tp / Tq: column-major temporaries like W / Wq (the column in
// M's row order while the rotations run).  W: (N + 1)^2, Wq: N^2; the merge owns the diagonal blocks at (off, off).
template <typename T>
__global__ __launch_bounds__(256) void svd_vectors_kernel(const int *merges, SvdWork<T> w, T *W, T *Tp, idx_t ldp, T *Wq, T *Tq, idx_t ldq,
							  int want_q, const int *status)
{
	__shared__ T red[4];
	if (status[0])
		return;
	const int b = blockIdx.y, kk = blockIdx.x, tid = threadIdx.x;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1], ks = merges[3 * b + 2];
	if (kk >= n)
		return;
	if (w.cnt[8 * b]) {
		// a zero node: identity factors
		for (int r = tid; r <= n; r += 256) {
			W[(off + r) + (off + kk) * ldp] = r == kk ? (T) 1 : (T) 0;
			if (kk == 0)
				W[(off + r) + (off + n) * ldp] = r == n ? (T) 1 : (T) 0;
		}
		if (want_q)
			for (int r = tid; r < n; r += 256)
				Wq[(off + r) + (off + kk) * ldq] = r == kk ? (T) 1 : (T) 0;
		return;
	}
	const int m = w.cnt[8 * b + 1], n0i = w.cnt[8 * b + 3], nij = w.cnt[8 * b + 4];
	const T cc0 = w.sc[4 * b], ss0 = w.sc[4 * b + 1];
	const T *dg = w.dg + off, *zh = w.zh + off;
	const int *op = w.op + off, *pm = w.pm + off, *jidx = w.jidx + off;
	const T *jc = w.jc + off, *js = w.js + off;
	const int col = w.colpos[off + kk];
	T *tp = Tp + off + (off + kk) * ldp, *tq = Tq + off + (off + kk) * ldq;
	for (int r = tid; r < n; r += 256) {
		tp[r] = 0;
		if (want_q)
			tq[r] = 0;
	}
	__syncthreads();
	if (zh[kk] == (T) 0) {
		if (tid == 0) {
			tp[op[kk]] = 1;
			if (want_q)
				tq[op[kk]] = 1;
		}
	} else {
		const T shift = w.sh[off + kk], mu = w.mu[off + kk];
		T mxu = 0, mxv = 0;
		for (int l = tid; l < m; l += 256) {
			const int i = pm[l];
			const T den = ((dg[i] - shift) - mu), den2 = dg[i] + (shift + mu);
			mxu = ev_max(mxu, ev_abs((zh[i] / den) / den2));
			mxv = ev_max(mxv, l == 0 ? (T) 1 : ev_abs(((dg[i] * zh[i]) / den) / den2));
		}
		mxu = block_reduce<T, true>(mxu, red);
		mxv = block_reduce<T, true>(mxv, red);
		const T iu = mxu > (T) 0 ? (T) 1 / mxu : (T) 1, iv = mxv > (T) 0 ? (T) 1 / mxv : (T) 1;
		T su = 0, sv = 0;
		for (int l = tid; l < m; l += 256) {
			const int i = pm[l];
			const T den = ((dg[i] - shift) - mu), den2 = dg[i] + (shift + mu);
			const T u = ((zh[i] / den) / den2) * iu;
			const T v = (l == 0 ? (T) -1 : ((dg[i] * zh[i]) / den) / den2) * iv;
			su += u * u;
			sv += v * v;
		}
		su = block_reduce<T, false>(su, red);
		sv = block_reduce<T, false>(sv, red);
		const T nu = (T) 1 / (mxu * ev_sqrt(su)), nv = (T) 1 / (mxv * ev_sqrt(sv));
		for (int l = tid; l < m; l += 256) {
			const int i = pm[l];
			const T den = ((dg[i] - shift) - mu), den2 = dg[i] + (shift + mu);
			tp[op[i]] = ((zh[i] / den) / den2) * nu;
			if (want_q)
				tq[op[i]] = (l == 0 ? (T) -1 : ((dg[i] * zh[i]) / den) / den2) * nv;
		}
	}
	__syncthreads();
	// the i-j rotations in reverse, then the 0-i ones in reverse (P only); one thread per factor walks its chain
	if (tid == 0 || (tid == 64 && want_q)) {
		T *x = tid == 0 ? tp : tq;
		for (int t = nij - 1; t >= 0; --t) {
			const int i = jidx[n0i + t];
			const int ra = op[i - 1], rb = op[i];
			const T c = jc[n0i + t], s = js[n0i + t];
			const T xv = x[rb], yv = x[ra]; // apply_on_the_left_in_place((row j, row i))
			x[rb] = c * xv - s * yv;
			x[ra] = c * yv + s * xv;
		}
		if (tid == 0 && n0i > 0) {
			T y = x[0];
			for (int t = n0i - 1; t >= 0; --t) {
				const int i = jidx[t];
				const T c = jc[t], s = js[t];
				const T xv = x[i];
				x[i] = c * xv - s * y;
				y = c * y + s * xv;
			}
			x[0] = y;
		}
	}
	__syncthreads();
	// rows of M -> rows of the children: M's row 0 is row k of the first child (times c0) and the last row of the second
	// (times s0) for P, row k for Q; rows 1 .. k go to 0 .. k - 1
	T *wc = W + off + (off + col) * ldp, *wq = Wq + off + (off + col) * ldq;
	for (int r = tid; r < n; r += 256) {
		const T x = tp[r];
		if (r == 0) {
			wc[ks] = cc0 * x;
			wc[n] = ss0 * x;
		} else {
			wc[r <= ks ? r - 1 : r] = x;
		}
		if (want_q)
			wq[r == 0 ? ks : (r <= ks ? r - 1 : r)] = tq[r];
	}
	if (kk == 0) {
		T *wl = W + off + (off + n) * ldp;
		for (int r = tid; r <= n; r += 256)
			wl[r] = r == ks ? -ss0 : (r == n ? cc0 : (T) 0);
	}
}

// ---- output -------------------------------------------------------------------------------------
// dst (m x nc) <- src (n x n, column major) in its top left corner, zero elsewhere, ones on the rest of the diagonal
// (mod.rs:405-411)
template <typename T> __global__ void svd_place_kernel(T *dst, idx_t rs, idx_t cs, idx_t m, idx_t nc, const T *src, idx_t lds, idx_t n)
{
	const idx_t t = (idx_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= m * nc)
		return;
	const idx_t i = t % m, j = t / m;
	dst[i * rs + j * cs] = i < n && j < n ? src[i + j * lds] : (i == j ? (T) 1 : (T) 0);
}

// The SVD of a tall or square device matrix M (m >= n >= 1) through its bidiagonal form (mod.rs:326-431, svd_imp).
// Uo: m x nu (nu = n or m) or .p == nullptr, Vo: n x n or .p == nullptr; S with stride ss.  Launches only; `status` is read by
// the caller.  `upper`: only the upper triangle of M is read (the R factor of the QR pre-step).
template <typename T>
void svd_squareish(MatV<const T> M, bool upper, MatV<T> Uo, MatV<T> Vo, T *S, idx_t ss, idx_t leaf, idx_t bs, int *status)
{
	const idx_t m = M.nrows, n = M.ncols;
	hipStream_t s = ctx().stream;
	const bool want_u = Uo.p != nullptr, want_v = Vo.p != nullptr;
	const int want_q = want_u ? 1 : 0;

	const DncPlan plan(n, leaf, 1, "svd: too many nodes");
	const int levels = plan.levels();

	const idx_t n1 = n + 1;
	const size_t pp = (size_t) n1 * (size_t) n1, qq = (size_t) n * (size_t) n;
	Scratch xb((size_t) m * (size_t) n * sizeof(T)), hlb((size_t) bs * (size_t) n * sizeof(T)), hrb((size_t) bs * (size_t) n * sizeof(T));
	Scratch pb0(pp * sizeof(T)), pb1(levels > 0 ? pp * sizeof(T) : 16), wb(levels > 0 ? pp * sizeof(T) : 16), tpb(levels > 0 ? pp * sizeof(T) : 16);
	Scratch qb0(want_q ? qq * sizeof(T) : 16), qb1(want_q && levels > 0 ? qq * sizeof(T) : 16), wqb(want_q && levels > 0 ? qq * sizeof(T) : 16),
		tqb(want_q && levels > 0 ? qq * sizeof(T) : 16);
	Scratch vec((size_t) 19 * (size_t) n1 * sizeof(T) + (size_t) 14 * (size_t) n1 * sizeof(int) + 64), tb(plan.tab_bytes() + 16);
	T *D0 = vec.as<T>(), *E0 = D0 + n1, *D = E0 + n1;
	SvdWork<T> w;
	{
		T *p = D + n1;
		dnc_carve(p, n1, {&w.dt, &w.ct, &w.dg, &w.c0, &w.dp, &w.zp, &w.sh, &w.mu, &w.sv, &w.zh, &w.jc, &w.js});
		w.sc = p;
		p += 4 * n1;
		int *ip = reinterpret_cast<int *>(p);
		dnc_carve(ip, n1, {&w.op, &w.pm, &w.nxt, &w.jidx, &w.colpos, &w.tmp});
		w.cnt = ip;
	}
	int *tab_dev = tb.as<int>();
	plan.upload(tab_dev, s);

	// B = Ul^H M Ur, diag / superdiag (mod.rs:347-392)
	MatV<T> X{xb.as<T>(), m, n, 1, m};
	typedef typename FloatBits<T>::U Bits;
	Bits *amax = reinterpret_cast<Bits *>(status + 4); // {max |M|, max(|d|, |e|)}
	T *fac = reinterpret_cast<T *>(status + 8);	    // their power-of-two factors
	FH_HIP(hipMemsetAsync(status + 4, 0, 12 * sizeof(int), s));
	const idx_t mn = m * n;
	hipLaunchKernelGGL(dnc_copy_kernel<T>, dim3(blocks_for(mn, 256)), dim3(256), 0, s, M.p, M.rs, M.cs, X.p, m, n, (int) (upper ? DNC_UPPER : DNC_ALL),
			   amax);
	hipLaunchKernelGGL(dnc_scale_kernel<T>, dim3(blocks_for(mn, 256)), dim3(256), 0, s, X.p, mn, (const Bits *) amax, fac);
	MatV<T> Hl{hlb.as<T>(), bs, n, 1, bs}, Hr{hrb.as<T>(), bs, n - 1, 1, bs};
	bidiag_dev<T>(X, Hl, Hr);
	hipLaunchKernelGGL(dnc_extract_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const T *) X.p, m, m, n, D0, E0, amax + 1, status);
	hipLaunchKernelGGL(dnc_tscale_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, D0, E0, n, (const Bits *) (amax + 1), fac + 1);

	// bidiagonal divide and conquer (factors of depth d: d even -> buffer 0, odd -> buffer 1; the root writes buffer 0)
	MatV<T> p0{pb0.as<T>(), n1, n1, 1, n1}, p1{pb1.as<T>(), n1, n1, 1, n1}, W{wb.as<T>(), n1, n1, 1, n1};
	MatV<T> q0{qb0.as<T>(), n, n, 1, n}, q1{qb1.as<T>(), n, n, 1, n}, Wq{wqb.as<T>(), n, n, 1, n};
	raise_dynamic_lds<&svd_leaf_kernel<T>>(svd_leaf_lds<T>(SVD_LEAF_MAX));
	hipLaunchKernelGGL(svd_leaf_kernel<T>, dim3((unsigned) plan.leaves.size()), dim3(64), svd_leaf_lds<T>((int) leaf), s, (const int *) tab_dev,
			   (const T *) D0, (const T *) E0, D, p0.p, p1.p, n1, q0.p, q1.p, n, want_q, status);
	for (int lv = levels - 1; lv >= 0; --lv) {
		const std::vector<DncNode> &ms = plan.merges[(size_t) lv];
		const int *mt = tab_dev + plan.level_at[(size_t) lv];
		const unsigned cnt = (unsigned) ms.size();
		const idx_t maxn = plan.maxn[(size_t) lv];
		const MatV<T> ps = (lv & 1) ? p0 : p1, pd = (lv & 1) ? p1 : p0; // children at depth lv + 1
		const MatV<T> qs = (lv & 1) ? q0 : q1, qd = (lv & 1) ? q1 : q0;
		hipLaunchKernelGGL(svd_merge_prep_kernel<T>, dim3(cnt), dim3(256), 0, s, mt, (const T *) D0, (const T *) E0, (const T *) D,
				   (const T *) ps.p, n1, w, (const int *) status);
		hipLaunchKernelGGL(svd_secular_kernel<T>, dim3(blocks_for(maxn, 4), cnt), dim3(256), 0, s, mt, w, (const int *) status);
		hipLaunchKernelGGL(svd_zhat_kernel<T>, dim3(blocks_for(maxn, 256), cnt), dim3(256), 0, s, mt, w, D, (const int *) status);
		hipLaunchKernelGGL(svd_vectors_kernel<T>, dim3((unsigned) maxn, cnt), dim3(256), 0, s, mt, w, W.p, tpb.as<T>(), n1, Wq.p, tqb.as<T>(), n,
				   want_q, (const int *) status);
		FH_HIP(hipGetLastError());
		for (const DncNode &mg : ms) {
			const idx_t o = mg.off, nn = mg.n, k = nn / 2, rem = nn - k - 1;
			gemm_dev<T>(pd.sub(o, o, k + 1, nn + 1), DST_FULL, false, ps.sub(o, o, k + 1, k + 1).c(), W.sub(o, o, k + 1, nn + 1).c(), (T) 1);
			gemm_dev<T>(pd.sub(o + k + 1, o, rem + 1, nn + 1), DST_FULL, false, ps.sub(o + k + 1, o + k + 1, rem + 1, rem + 1).c(),
				    W.sub(o + k + 1, o, rem + 1, nn + 1).c(), (T) 1);
			if (want_q) {
				gemm_dev<T>(qd.sub(o, o, k, nn), DST_FULL, false, qs.sub(o, o, k, k).c(), Wq.sub(o, o, k, nn).c(), (T) 1);
				copy_dev<T>(qd.sub(o + k, o, 1, nn), Wq.sub(o + k, o, 1, nn).c());
				gemm_dev<T>(qd.sub(o + k + 1, o, rem, nn), DST_FULL, false, qs.sub(o + k + 1, o + k + 1, rem, rem).c(),
					    Wq.sub(o + k + 1, o, rem, nn).c(), (T) 1);
			}
		}
	}

	// U = Ul [Q 0; 0 I], V = Ur [1 0; 0 .] P[0:n, 0:n] (mod.rs:403-429)
	if (want_u) {
		hipLaunchKernelGGL(svd_place_kernel<T>, dim3(blocks_for(m * Uo.ncols, 256)), dim3(256), 0, s, Uo.p, Uo.rs, Uo.cs, m, Uo.ncols,
				   (const T *) q0.p, n, n);
		apply_householder_sequence_left_dev<T>(X.c(), Hl.c(), Uo, false);
	}
	if (want_v) {
		hipLaunchKernelGGL(svd_place_kernel<T>, dim3(blocks_for(n * n, 256)), dim3(256), 0, s, Vo.p, Vo.rs, Vo.cs, n, n, (const T *) p0.p, n1, n);
		if (n > 1)
			apply_householder_sequence_left_dev<T>(X.sub(0, 1, n - 1, n - 1).t().c(), Hr.c(), Vo.sub(1, 0, n - 1, n), false);
	}
	hipLaunchKernelGGL(dnc_write_s_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const T *) D, n, S, ss, (const T *) fac);
	FH_HIP(hipGetLastError());
	FH_HIP(hipStreamSynchronize(s)); // the plan and the scratch of this frame stay alive until their work has run
}

} // namespace

// Leaves of min(max(recursion_threshold, 4), 64) entries for both dtypes (the header comment has the LDS budget).
idx_t svd_leaf_size(size_t recursion_threshold) { return dnc_leaf_size(recursion_threshold, SVD_LEAF_MAX); }

template <typename T> void svd_identity_dev(MatV<T> X)
{
	if (X.nrows == 0 || X.ncols == 0)
		return;
	hipLaunchKernelGGL(svd_place_kernel<T>, dim3(blocks_for(X.nrows * X.ncols, 256)), dim3(256), 0, ctx().stream, X.p, X.rs, X.cs, X.nrows,
			   X.ncols, (const T *) nullptr, (idx_t) 0, (idx_t) 0);
	FH_HIP(hipGetLastError());
}
template void svd_identity_dev<double>(MatV<double>);
template void svd_identity_dev<float>(MatV<float>);

template <typename T>
int svd_dev(MatV<const T> A, MatV<T> U, MatV<T> V, T *S, idx_t ss, idx_t leaf, double qr_ratio_threshold, idx_t qr_blocking_threshold,
	    idx_t bs_mn, idx_t bs_nn)
{
	if (A.ncols > A.nrows) { // mod.rs:580-584
		A = A.t();
		std::swap(U, V);
	}
	const idx_t m = A.nrows, n = A.ncols;
	FH_CHECK(n > 0, "svd: the matrix must not be empty");
	FH_CHECK(m < (1L << 30), "svd: matrix too large");
	FH_CHECK(leaf >= 4 && leaf <= SVD_LEAF_MAX, "svd: leaf size out of range");
	hipStream_t s = ctx().stream;
	Scratch stb(16 * sizeof(int));
	int *status = stb.as<int>();
	FH_HIP(hipMemsetAsync(status, 0, 16 * sizeof(int), s));
	if ((double) m / (double) n <= qr_ratio_threshold) {
		svd_squareish<T>(A, false, U, V, S, ss, leaf, bs_mn, status);
	} else {
		// mod.rs:604-661: A = Q R, the SVD of R, U <- Q [U_R; 0 (I)]
		Scratch xb((size_t) m * (size_t) n * sizeof(T)), hb((size_t) bs_mn * (size_t) n * sizeof(T));
		MatV<T> X{xb.as<T>(), m, n, 1, m}, H{hb.as<T>(), bs_mn, n, 1, bs_mn};
		copy_dev<T>(X, A);
		geqrf_dev<T>(X, H, qr_blocking_threshold);
		const bool want_u = U.p != nullptr;
		Scratch ub(want_u ? (size_t) n * (size_t) n * sizeof(T) : 16);
		const MatV<T> Ur{want_u ? ub.as<T>() : nullptr, n, n, 1, n};
		svd_squareish<T>(X.sub(0, 0, n, n).c(), true, Ur, V, S, ss, leaf, bs_nn, status);
		if (want_u) {
			hipLaunchKernelGGL(svd_place_kernel<T>, dim3(blocks_for(m * U.ncols, 256)), dim3(256), 0, s, U.p, U.rs, U.cs, m, U.ncols,
					   (const T *) Ur.p, n, n);
			FH_HIP(hipGetLastError());
			apply_householder_sequence_left_dev<T>(X.c(), H.c(), U, false);
		}
	}
	return dnc_read_status(status, s);
}

template int svd_dev<double>(MatV<const double>, MatV<double>, MatV<double>, double *, idx_t, idx_t, double, idx_t, idx_t, idx_t);
template int svd_dev<float>(MatV<const float>, MatV<float>, MatV<float>, float *, idx_t, idx_t, double, idx_t, idx_t, idx_t);

} // namespace fh
