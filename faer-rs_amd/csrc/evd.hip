// Self-adjoint eigendecomposition -- faer/src/linalg/evd/mod.rs:270-425 (self_adjoint_evd) with the divide and
// conquer solver of the symmetric tridiagonal problem, evd/tridiag_evd.rs:270-660, on the device.
//
//   copy lower(A) -> tridiag_dev (condense.hip) -> diag / offdiag -> tridiagonal solve -> block Householder back-transform
//   (apply_householder_sequence_left_dev) -> S.
//
// The tridiagonal solve follows the reference's recursion (split at n / 2, rank-one tear d[n1-1] -= |rho|, d[n1] -= |rho|)
// but runs it level by level, bottom up; every launch covers all nodes of one level:
//   * evd_leaf_kernel: implicit symmetric QR with the Wilkinson shift (tridiag_evd.rs:9-190) on every leaf of at most
//     min(max(recursion_threshold, 4), 64) rows (evd_leaf_size), one single-wave workgroup per leaf, one row per lane, the
//     leaf's eigenvector block in LDS (64 x 65 fp64 = 32.5 KiB at most).  Lane 0 generates a sweep's Givens rotations; then
//     every lane applies the whole sweep to its row of U (rotations on the right act on each row on its own: one barrier
//     per sweep).
//   * evd_merge_prep_kernel (one workgroup per merge): z from the last row of U0 and the first row of U1, the merge of
//     the two ascending halves (pl_before), deflation of small rho z_i and of runs of nearly equal d (Householder
//     reflector as the reference), compaction of the k non-deflated entries (:370-480).
//   * evd_secular_kernel (one wavefront per root): the reference's secular_eq_root_finder (svd/bidiag_svd.rs:7); a root
//     is kept as (pole, mu) so that lambda_j - d_i = (d_i - pole_j) - mu_j never cancels.
//   * evd_loewner_kernel (one thread per entry): Gu-Eisenstat z-hat recomputed from the roots, and the ascending order of
//     the merged eigenvalues (pr).
//   * evd_qhat_kernel (one workgroup per column): the reference's repaired_u in the final column order, deflated columns
//     as unit vectors, the run reflectors applied, rows mapped back through pl_before.
//   * two MFMA products per merge on gemm_dev: U[0:n1, :] = U0 Qhat_top, U[n1:, :] = U1 Qhat_bot (:595-598).
// The shapes of every launch follow from n alone (deflation only changes the contents of Qhat), so the solve has no
// host synchronization; the call reads back one status word at its end.
#include <cmath>

#include "common.h"
#include "dnc.h"

namespace fh {

namespace {

// per-level work vectors (n entries each, a merge at offset `off` owns [off, off + its size)); per-merge scalars by the
// merge's index in its level
template <typename T> struct EvdWork {
	T *z, *pd0, *pz0, *pd, *pz, *hh, *mu, *sh, *zh;
	int *plb, *pla, *rl, *pr;
	int *k, *applied;
	T *rho;
};

// rank-one tears of every merge (tridiag_evd.rs:290-296).  With leaves of at least 4 rows no two merges touch the same entry.
template <typename T> __global__ void evd_tear_kernel(const int *merges, int count, T *D, const T *E, const int *status)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= count || status[0])
		return;
	const idx_t off = merges[3 * t], n1 = merges[3 * t + 2];
	const T r = ev_abs(E[off + n1 - 1]);
	D[off + n1 - 1] -= r;
	D[off + n1] -= r;
}

// ---- leaves: QR algorithm -----------------------------------------------------------------------
constexpr int EVD_LEAF_MAX = 64; // one row per lane

// highest index < lim whose bit is set in the mask, -1 if none
__device__ __forceinline__ int highest_below(unsigned long long mask, int lim)
{
	if (lim <= 0)
		return -1;
	const unsigned long long l = lim >= 64 ? mask : mask & ((1ull << lim) - 1ull);
	return l ? 63 - __clzll((long long) l) : -1;
}

template <typename T> constexpr size_t evd_leaf_lds(int m) { return ((size_t) m * (m + 1) + 4 * EVD_LEAF_MAX) * sizeof(T) + EVD_LEAF_MAX * sizeof(int); }

// one wavefront per leaf; leaves[3 * b ..]: offset, rows, destination buffer (0: U0, 1: U1)
template <typename T>
__global__ __launch_bounds__(64) void evd_leaf_kernel(const int *leaves, T *D, const T *E, T *U0, idx_t rs0, idx_t cs0, T *U1, idx_t rs1,
						      idx_t cs1, int *status)
{
	extern __shared__ __align__(16) unsigned char evd_lds[];
	const int tid = threadIdx.x;
	const idx_t off = leaves[3 * blockIdx.x];
	const int m = leaves[3 * blockIdx.x + 1];
	T *Ug = leaves[3 * blockIdx.x + 2] ? U1 : U0;
	const idx_t rs = leaves[3 * blockIdx.x + 2] ? rs1 : rs0, cs = leaves[3 * blockIdx.x + 2] ? cs1 : cs0;
	if (status[0])
		return;
	const int ld = m + 1;
	T *u = reinterpret_cast<T *>(evd_lds); // row major, u[i * ld + j] = U(i, j): lane i owns row i
	T *d = u + (size_t) m * ld, *e = d + EVD_LEAF_MAX, *rc = e + EVD_LEAF_MAX, *rsn = rc + EVD_LEAF_MAX;
	int *perm = reinterpret_cast<int *>(rsn + EVD_LEAF_MAX);
	__shared__ int sh_kend;
	const T eps = DncTraits<T>::eps, sml = DncTraits<T>::sml;

	for (int t = tid; t < m * ld; t += 64)
		u[t] = (t % ld) == (t / ld) ? (T) 1 : (T) 0;
	for (int i = tid; i < m; i += 64) {
		d[i] = D[off + i];
		e[i] = i + 1 < m ? E[off + i] : (T) 0;
		perm[i] = i;
	}
	__syncthreads();
	T scale = 1;
	bool fail = false;
	if (m == 2) {
		// tridiag_evd.rs:27-82
		if (tid == 0) {
			const T a = d[0], dd = d[1], b = e[0], half = (T) 0.5;
			const T t0 = ev_hypot(a - dd, b * (T) 2) * half, t1 = (a + dd) * half;
			const T r0 = t1 - t0, r1 = t1 + t0;
			const T tol = ev_max(ev_abs(r0), ev_abs(r1)) * eps;
			T u00 = 1, u10 = 0, u01 = 0, u11 = 1;
			if (r1 - r0 <= tol) {
			} else if (ev_abs(b) <= tol) {
				if (!(d[0] < d[1])) {
					u00 = 0;
					u10 = 1;
					u01 = 1;
					u11 = 0;
				}
			} else {
				const T tau = ((dd - a) / b) * half;
				T t = (T) 1 / (ev_abs(tau) + ev_hypot(tau, (T) 1));
				if (tau < (T) 0)
					t = -t;
				T c = ev_hypot(t, (T) 1);
				T s = c * t;
				const T r = ev_hypot(c, s);
				c = c / r;
				s = s / r;
				const T r0_r = (c * a - s * b) / c;
				if (ev_abs(r0 - r0_r) < r1 - r0_r) {
					u00 = c;
					u10 = -s;
					u01 = s;
					u11 = c;
				} else {
					u01 = c;
					u11 = -s;
					u00 = s;
					u10 = c;
				}
			}
			u[0] = u00;
			u[1] = u01;
			u[ld] = u10;
			u[ld + 1] = u11;
			d[0] = r0;
			d[1] = r1;
		}
		__syncthreads();
	} else if (m > 2) {
		// tridiag_evd.rs:84-190
		T mx = 0;
		for (int i = tid; i < m; i += 64)
			mx = ev_max(mx, ev_max(ev_abs(d[i]), ev_abs(e[i])));
		mx = wave_max(mx);
		if (mx != (T) 0) {
			scale = mx;
			const T inv = (T) 1 / mx;
			for (int i = tid; i < m; i += 64) {
				d[i] *= inv;
				e[i] *= inv;
			}
			__syncthreads();
			int start = 0, end = m - 1;
			const long max_iters = DncTraits<T>::iter_factor * (long) m * (long) m;
			for (long iter = 0; iter < max_iters; ++iter) {
				for (int i = start + tid; i < end; i += 64) {
					const T ei = ev_abs(e[i]);
					if (ei < sml || ei < eps * ev_hypot(d[i], d[i + 1]))
						e[i] = 0;
				}
				__syncthreads();
				const bool v0 = tid < m - 1;
				const T e0 = v0 ? e[tid] : (T) 0;
				const unsigned long long nz0 = __ballot(v0 && e0 != (T) 0), z0 = __ballot(v0 && e0 == (T) 0);
				end = highest_below(nz0, end) + 1; // while end > 0 && offdiag[end - 1] == 0: end -= 1
				if (end == 0)
					break;
				if (iter + 1 == max_iters) {
					fail = true;
					break;
				}
				start = highest_below(z0, end - 1) + 1; // while start > 0 && offdiag[start - 1] != 0: start -= 1
				if (tid == 0) {
					const T td = (d[end - 1] - d[end]) * (T) 0.5;
					const T ee = e[end - 1];
					T mu = d[end];
					if (td == (T) 0) {
						mu -= ev_abs(ee);
					} else if (ee != (T) 0) {
						const T e2 = ee * ee;
						T h = ev_hypot(td, ee);
						if (!(td > (T) 0))
							h = -h;
						if (e2 == (T) 0)
							mu = mu - ee / ((td + h) / ee);
						else
							mu = mu - e2 / (td + h);
					}
					T x = d[start] - mu, z = e[start];
					int k = start;
					T dk = d[k], ek = e[k];
					while (k < end && z != (T) 0) {
						T c, s;
						make_givens(x, z, c, s);
						const T dk1 = d[k + 1];
						const T sdk = s * dk + c * ek;
						const T dkp1 = s * ek + c * dk1;
						d[k] = c * (c * dk - s * ek) - s * (c * ek - s * dk1);
						const T nd1 = s * sdk + c * dkp1;
						const T nek = c * sdk - s * dkp1;
						d[k + 1] = nd1;
						e[k] = nek;
						if (k > start)
							e[k - 1] = c * e[k - 1] - s * z;
						x = nek;
						T ek1 = e[k + 1];
						if (k < end - 1) {
							z = -s * ek1;
							ek1 = c * ek1;
							e[k + 1] = ek1;
						}
						rc[k] = c;
						rsn[k] = s;
						dk = nd1;
						ek = ek1;
						++k;
					}
					sh_kend = k;
				}
				__syncthreads();
				const int kend = sh_kend;
				for (int i = tid; i < m; i += 64)
					rot_chain_forward(u + (size_t) i * ld, start, kend, rc, rsn);
				__syncthreads();
			}
			if (!fail && tid == 0) {
				// selection sort with column swaps (:170-186)
				for (int i = 0; i < m - 1; ++i) {
					int idx = i;
					T mn = d[i];
					for (int k = i + 1; k < m; ++k)
						if (d[k] < mn) {
							idx = k;
							mn = d[k];
						}
					if (idx != i) {
						const T a = d[i];
						d[i] = d[idx];
						d[idx] = a;
						const int p = perm[i];
						perm[i] = perm[idx];
						perm[idx] = p;
					}
				}
			}
			__syncthreads();
		}
	}
	if (fail) {
		if (tid == 0)
			status[0] = 1;
		return;
	}
	for (int i = tid; i < m; i += 64)
		D[off + i] = d[i] * scale;
	for (int t = tid; t < m * m; t += 64) {
		const int i = t % m, j = t / m;
		Ug[(off + i) * rs + (off + j) * cs] = u[(size_t) i * ld + perm[j]];
	}
}

// ---- merges ---------------------------------------------------------------------------------------
// merges[3 * b ..]: offset, size n, n1 (the first half)
template <typename T>
__global__ __launch_bounds__(256) void evd_merge_prep_kernel(const int *merges, const T *D, const T *E, const T *Uc, idx_t rs, idx_t cs,
							     EvdWork<T> w, const int *status)
{
	__shared__ T red[4];
	__shared__ int applied_sh;
	__shared__ int scan[257];
	if (status[0])
		return;
	const int b = blockIdx.x, tid = threadIdx.x;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1], n1 = merges[3 * b + 2], n2 = n - n1;
	const T eps = DncTraits<T>::eps, sml = DncTraits<T>::sml;
	const T rho_in = E[off + n1 - 1];
	const bool neg = rho_in < (T) 0;
	const T inv_sqrt2 = ev_sqrt((T) 0.5);
	const T *d = D + off;
	T *z = w.z + off, *pd0 = w.pd0 + off, *pz0 = w.pz0 + off;
	int *plb = w.plb + off, *rl = w.rl + off;
	if (tid == 0)
		applied_sh = 0;
	// z (tridiag_evd.rs:370-380) and pl_before (:382-397): the merge position of an entry of either ascending half is its
	// index plus the entries of the other half that precede it (a tie takes the second half first)
	for (int i = tid; i < n; i += 256) {
		T uv;
		int pos;
		if (i < n1) {
			uv = Uc[(off + n1 - 1) * rs + (off + i) * cs];
			const T x = d[i];
			int lo = 0, hi = n2; // count of d1[j] <= x
			while (lo < hi) {
				const int mid = (lo + hi) >> 1;
				if (d[n1 + mid] <= x)
					lo = mid + 1;
				else
					hi = mid;
			}
			pos = i + lo;
		} else {
			uv = Uc[(off + n1) * rs + (off + i) * cs];
			if (neg)
				uv = -uv;
			const T x = d[i];
			int lo = 0, hi = n1; // count of d0[p] < x
			while (lo < hi) {
				const int mid = (lo + hi) >> 1;
				if (d[mid] < x)
					lo = mid + 1;
				else
					hi = mid;
			}
			pos = (i - n1) + lo;
		}
		z[i] = uv * inv_sqrt2;
		plb[pos] = i;
	}
	__syncthreads();
	const T rho = ev_abs(rho_in) * (T) 2;
	T dm = 0, zm = 0;
	for (int i = tid; i < n; i += 256) {
		const int p = plb[i];
		const T dv = d[p], zv = z[p];
		pd0[i] = dv;
		pz0[i] = zv;
		dm = ev_max(dm, ev_abs(dv));
		zm = ev_max(zm, ev_abs(zv));
	}
	const T dmax = block_reduce<T, true>(dm, red);
	const T zmax = block_reduce<T, true>(zm, red);
	const T tol = (T) 8 * eps * ev_max(dmax, zmax);
	const bool all_deflated = rho * zmax <= tol; // :404-418
	if (!all_deflated) {
		for (int i = tid; i < n; i += 256) {
			if (ev_abs(rho * pz0[i]) <= tol)
				pz0[i] = 0;
			// a gap above tol always starts a run (the entries are ascending): mark the segments that the walkers below own
			rl[i] = (i == 0 || pd0[i] - pd0[i - 1] > tol) ? -1 : 0;
		}
		__syncthreads();
		// runs of nearly equal d (:424-452), one walker per segment.  A run is measured from its first entry, so a segment may
		// hold several runs: a walker starts only at a segment mark (-1), which no other thread overwrites (the walkers write
		// run lengths >= 1 at run starts and 0 inside runs; the next segment's mark stays nonzero and stops the walk)
		for (int i = tid; i < n; i += 256) {
			if (rl[i] != -1)
				continue;
			int idx = i;
			while (true) {
				int run_len = 1;
				const T d_prev = pd0[idx];
				while (idx + run_len < n && pd0[idx + run_len] - d_prev <= tol) {
					pd0[idx + run_len] = d_prev;
					rl[idx + run_len] = 0;
					++run_len;
				}
				rl[idx] = run_len;
				if (run_len > 1) {
					applied_sh = 1;
					T *hh = w.hh + off + idx, *zr = pz0 + idx;
					T head = zr[run_len - 1];
					T tn = 0;
					for (int t = 0; t < run_len - 1; ++t)
						tn += zr[t] * zr[t];
					tn = ev_sqrt(tn);
					T head_norm = ev_abs(head);
					if (head_norm < sml) {
						head = 0;
						head_norm = 0;
					}
					T tau;
					if (tn < sml) {
						// make_householder_in_place: tau = inf, the reflector is the identity
						tau = ev_inf<T>();
						for (int t = 0; t < run_len - 1; ++t)
							hh[t] = zr[t];
					} else {
						const T nrm = ev_hypot(head_norm, tn);
						const T sign = head_norm != (T) 0 ? head / head_norm : (T) 1;
						const T signed_norm = sign * nrm;
						const T hwb_inv = (T) 1 / (head + signed_norm);
						for (int t = 0; t < run_len - 1; ++t)
							hh[t] = zr[t] * hwb_inv;
						head = -signed_norm;
						const T q = tn * ev_abs(hwb_inv);
						tau = (T) 0.5 * ((T) 1 + q * q);
					}
					for (int t = 0; t < run_len - 1; ++t)
						zr[t] = 0;
					zr[run_len - 1] = head;
					hh[run_len - 1] = tau;
				}
				idx += run_len;
				if (idx >= n || rl[idx] != 0)
					break;
			}
		}
	}
	__syncthreads();
	// stable compaction: the k entries with z != 0 first, the deflated ones after them (:453-476)
	const int chunk = (n + 255) / 256;
	const int c0 = tid * chunk < n ? tid * chunk : n, c1 = c0 + chunk < n ? c0 + chunk : n;
	int cnt = 0;
	if (!all_deflated)
		for (int i = c0; i < c1; ++i)
			cnt += pz0[i] != (T) 0;
	scan[tid + 1] = cnt;
	__syncthreads();
	if (tid == 0) {
		scan[0] = 0;
		for (int t = 1; t <= 256; ++t)
			scan[t] += scan[t - 1];
	}
	__syncthreads();
	const int k = scan[256];
	int wn = scan[tid], wd = k + (c0 - scan[tid]);
	for (int i = c0; i < c1; ++i) {
		const T zv = pz0[i];
		if (!all_deflated && zv != (T) 0) {
			w.pd[off + wn] = pd0[i];
			w.pz[off + wn] = zv;
			w.pla[off + wn] = i;
			++wn;
		} else {
			w.pd[off + wd] = pd0[i];
			w.pla[off + wd] = i;
			++wd;
		}
	}
	if (tid == 0) {
		w.k[b] = k;
		w.applied[b] = all_deflated ? 0 : applied_sh;
		w.rho[b] = rho;
	}
}

// compute_eigenvalues (tridiag_evd.rs:233-268): one wavefront per root; grid (ceil(max n / 4), merges)
template <typename T> __global__ __launch_bounds__(256) void evd_secular_kernel(const int *merges, EvdWork<T> w, const int *status)
{
	if (status[0])
		return;
	const int b = blockIdx.y;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1];
	const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (i >= n)
		return;
	const int k = w.k[b];
	if (i >= k) {
		if ((threadIdx.x & 63) == 0) {
			w.sh[off + i] = 0;
			w.mu[off + i] = w.pd[off + i];
		}
		return;
	}
	const T rho = w.rho[b];
	const T *d = w.pd + off, *z = w.pz + off;
	const bool last = i == k - 1;
	T right;
	if (last) {
		T acc = 0;
		for (int t = (int) (threadIdx.x & 63); t < k; t += 64)
			acc += z[t] * z[t];
		right = d[i] + rho * wave_sum(acc);
	} else {
		right = d[i + 1];
	}
	SecularEq<T> f{d, z, k, (T) 1 / rho};
	T shift, mu;
	secular_root<T>(f, d[i], right, last, shift, mu);
	if ((threadIdx.x & 63) == 0) {
		w.sh[off + i] = shift;
		w.mu[off + i] = mu;
	}
}

// Loewner z-hat (:497-511) and the ascending order of the merged eigenvalues (:516-533); grid (ceil(max n / 256), merges)
template <typename T> __global__ __launch_bounds__(256) void evd_loewner_kernel(const int *merges, EvdWork<T> w, T *D, const int *status)
{
	if (status[0])
		return;
	const int b = blockIdx.y;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1];
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const int k = w.k[b];
	const T *mu = w.mu + off, *sh = w.sh + off, *d = w.pd + off;
	if (i < k) {
		const T di = d[i];
		T prod = mu[i] + (sh[i] - di);
		for (int t = 0; t < k; ++t)
			if (t != i)
				prod *= (mu[t] + (sh[t] - di)) / (d[t] - di);
		prod = ev_sqrt(ev_abs(prod));
		w.zh[off + i] = w.pz[off + i] < (T) 0 ? -prod : prod;
	}
	const T lam = mu[i] + sh[i];
	int rank = 0;
	for (int t = 0; t < n; ++t) {
		const T lt = mu[t] + sh[t];
		rank += (lt < lam) || (lt == lam && t < i);
	}
	w.pr[off + rank] = i;
	D[off + rank] = lam;
}

// repaired_u (:534-592) in the final column order; grid (max n, merges), one column per workgroup.  Q is N x N column major
// (ld N), the merge owns the diagonal block at (off, off).
template <typename T> __global__ __launch_bounds__(256) void evd_qhat_kernel(const int *merges, EvdWork<T> w, T *Q, idx_t ldq, const int *status)
{
	__shared__ T red[4];
	if (status[0])
		return;
	const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
	const idx_t off = merges[3 * b];
	const int n = merges[3 * b + 1];
	if (j >= n)
		return;
	const int k = w.k[b], pj = w.pr[off + j];
	const int *pla = w.pla + off, *plb = w.plb + off;
	T *q = Q + off + (off + j) * ldq;
	if (pj >= k) {
		for (int i = tid; i < n; i += 256)
			q[plb[pla[i]]] = i == pj ? (T) 1 : (T) 0;
	} else {
		const T mu = w.mu[off + pj], sh = w.sh[off + pj];
		const T *zh = w.zh + off, *d = w.pd + off;
		// norm_l2 with a scale: an entry next to a pole may be huge
		T mx = 0;
		for (int i = tid; i < k; i += 256)
			mx = ev_max(mx, ev_abs(zh[i] / ((d[i] - sh) - mu)));
		mx = block_reduce<T, true>(mx, red);
		const T inv_mx = mx > (T) 0 ? (T) 1 / mx : (T) 1;
		T ss = 0;
		for (int i = tid; i < k; i += 256) {
			const T v = (zh[i] / ((d[i] - sh) - mu)) * inv_mx;
			ss += v * v;
		}
		ss = block_reduce<T, false>(ss, red);
		const T inv_norm = (T) 1 / (mx * ev_sqrt(ss));
		for (int i = tid; i < n; i += 256)
			q[plb[pla[i]]] = i < k ? (zh[i] / ((d[i] - sh) - mu)) * inv_norm : (T) 0;
	}
	if (!w.applied[b])
		return;
	__syncthreads(); // the column's entries written by the other threads of the block
	// the run reflectors (:566-590); rows are in pl_before order, so row r of the picture sits at q[plb[r]]
	const int *rl = w.rl + off;
	const T *hh = w.hh + off;
	for (int r = tid; r < n; r += 256) {
		const int len = rl[r];
		if (len <= 1)
			continue;
		const T tau_inv = (T) 1 / hh[r + len - 1];
		T dot = 0;
		for (int t = 0; t < len; ++t)
			dot += (t + 1 < len ? hh[r + t] : (T) 1) * q[plb[r + t]];
		dot *= tau_inv;
		for (int t = 0; t < len; ++t)
			q[plb[r + t]] -= dot * (t + 1 < len ? hh[r + t] : (T) 1);
	}
}

} // namespace

// Leaves of min(max(recursion_threshold, 4), 64) rows, the most evd_leaf_kernel holds.  Lane 0's Givens chain grows as the
// square of the leaf size while the merge level that smaller leaves add is cheap: at N = 4096 fp64 the solve took 8.8 ms
// with 64-row leaves against 15.8 ms with the 128-row ones an earlier leaf kernel could hold (32: 8.6).
idx_t evd_leaf_size(size_t recursion_threshold) { return dnc_leaf_size(recursion_threshold, EVD_LEAF_MAX); }

template <typename T> int self_adjoint_evd_dev(MatV<const T> A, MatV<T> U, T *S, idx_t ss, idx_t leaf, idx_t bs)
{
	const idx_t n = A.nrows;
	FH_CHECK(A.ncols == n && n > 0, "self_adjoint_evd: the matrix must be square and not empty");
	FH_CHECK(n < (1L << 30), "self_adjoint_evd: matrix too large");
	FH_CHECK(leaf >= 4 && leaf <= EVD_LEAF_MAX, "self_adjoint_evd: leaf size out of range");
	hipStream_t s = ctx().stream;
	const bool want_u = U.p != nullptr;

	// plan of the recursion (host, from n alone)
	const DncPlan plan(n, leaf, 0, "self_adjoint_evd: too many nodes");
	const int levels = plan.levels();

	// device memory: the reduced matrix, its block factors, two eigenvector buffers (depth parity), Qhat, the work vectors
	const size_t nn = (size_t) n * (size_t) n;
	Scratch trid(nn * sizeof(T)), hb((size_t) bs * (size_t) (n > 1 ? n - 1 : 1) * sizeof(T));
	Scratch ub0(want_u ? 16 : nn * sizeof(T)), ub1(levels > 0 ? nn * sizeof(T) : 16), qb(levels > 0 ? nn * sizeof(T) : 16);
	Scratch vec((size_t) 12 * (size_t) n * sizeof(T) + (size_t) (4 * n + 2 * (n + 1)) * sizeof(int) + 64), tb(plan.tab_bytes() + 16),
		stb(16 * sizeof(int));
	int *status = stb.as<int>();
	T *D = vec.as<T>(), *E = D + n;
	EvdWork<T> w;
	{
		T *p = E + n;
		dnc_carve(p, n, {&w.z, &w.pd0, &w.pz0, &w.pd, &w.pz, &w.hh, &w.mu, &w.sh, &w.zh, &w.rho});
		int *ip = reinterpret_cast<int *>(p);
		dnc_carve(ip, n, {&w.plb, &w.pla, &w.rl, &w.pr});
		w.k = ip;
		w.applied = ip + (n + 1);
	}
	int *tab_dev = tb.as<int>();
	FH_HIP(hipMemsetAsync(status, 0, 16 * sizeof(int), s));
	plan.upload(tab_dev, s);

	// 1-3: T = Q^H lower(A) Q, diag / offdiag (mod.rs:326-356); the strict upper triangle of A is never read
	MatV<T> X{trid.as<T>(), n, n, 1, n};
	typedef typename FloatBits<T>::U Bits;
	Bits *amax = reinterpret_cast<Bits *>(status + 4); // {max |lower(A)|, max(|d|, |e|)}
	T *fac = reinterpret_cast<T *>(status + 8);	    // their power-of-two factors
	hipLaunchKernelGGL(dnc_copy_kernel<T>, dim3(blocks_for((idx_t) nn, 256)), dim3(256), 0, s, A.p, A.rs, A.cs, X.p, n, n, (int) DNC_LOWER, amax);
	hipLaunchKernelGGL(dnc_scale_kernel<T>, dim3(blocks_for((idx_t) nn, 256)), dim3(256), 0, s, X.p, (idx_t) nn, (const Bits *) amax, fac);
	MatV<T> H{hb.as<T>(), bs, n - 1, 1, bs};
	if (n > 1)
		tridiag_dev<T>(X, H);
	hipLaunchKernelGGL(dnc_extract_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const T *) X.p, n, (idx_t) 1, n, D, E, amax + 1, status);
	hipLaunchKernelGGL(dnc_tscale_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, D, E, n, (const Bits *) (amax + 1), fac + 1);

	// 4: tridiagonal divide and conquer (U buffer of depth d: d even -> u0, odd -> u1; the root writes u0)
	MatV<T> u0 = want_u ? U : MatV<T>{ub0.as<T>(), n, n, 1, n};
	MatV<T> u1{ub1.as<T>(), n, n, 1, n};
	if (plan.nmerges > 0)
		hipLaunchKernelGGL(evd_tear_kernel<T>, dim3(blocks_for((idx_t) plan.nmerges, 256)), dim3(256), 0, s, tab_dev + plan.level_at[0],
				   (int) plan.nmerges, D, E, status);
	raise_dynamic_lds<&evd_leaf_kernel<T>>(evd_leaf_lds<T>(EVD_LEAF_MAX));
	hipLaunchKernelGGL(evd_leaf_kernel<T>, dim3((unsigned) plan.leaves.size()), dim3(64), evd_leaf_lds<T>((int) leaf), s, tab_dev, D, E, u0.p, u0.rs,
			   u0.cs, u1.p, u1.rs, u1.cs, status);
	MatV<T> Q{qb.as<T>(), n, n, 1, n};
	for (int lv = levels - 1; lv >= 0; --lv) {
		const std::vector<DncNode> &ms = plan.merges[(size_t) lv];
		const int *mt = tab_dev + plan.level_at[(size_t) lv];
		const unsigned cnt = (unsigned) ms.size();
		const idx_t maxn = plan.maxn[(size_t) lv];
		const MatV<T> src = (lv & 1) ? u0 : u1, dst = (lv & 1) ? u1 : u0; // children at depth lv + 1
		hipLaunchKernelGGL(evd_merge_prep_kernel<T>, dim3(cnt), dim3(256), 0, s, mt, (const T *) D, (const T *) E, (const T *) src.p, src.rs,
				   src.cs, w, status);
		hipLaunchKernelGGL(evd_secular_kernel<T>, dim3(blocks_for(maxn, 4), cnt), dim3(256), 0, s, mt, w, status);
		hipLaunchKernelGGL(evd_loewner_kernel<T>, dim3(blocks_for(maxn, 256), cnt), dim3(256), 0, s, mt, w, D, status);
		hipLaunchKernelGGL(evd_qhat_kernel<T>, dim3((unsigned) maxn, cnt), dim3(256), 0, s, mt, w, Q.p, n, status);
		FH_HIP(hipGetLastError());
		for (const DncNode &m : ms) {
			const idx_t o = m.off, n1 = m.n / 2, n2 = m.n - n1;
			gemm_dev<T>(dst.sub(o, o, n1, m.n), DST_FULL, false, src.sub(o, o, n1, n1).c(), Q.sub(o, o, n1, m.n).c(), (T) 1);
			gemm_dev<T>(dst.sub(o + n1, o, n2, m.n), DST_FULL, false, src.sub(o + n1, o + n1, n2, n2).c(), Q.sub(o + n1, o, n2, m.n).c(),
				    (T) 1);
		}
	}

	// 5: U[1:, :] <- Q_tridiag U[1:, :] (mod.rs:410-418)
	if (want_u && n > 1)
		apply_householder_sequence_left_dev<T>(X.sub(1, 0, n - 1, n - 1).c(), H.c(), U.sub(1, 0, n - 1, n), false);
	// 6: S
	hipLaunchKernelGGL(dnc_write_s_kernel<T>, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const T *) D, n, S, ss, (const T *) fac);
	FH_HIP(hipGetLastError());
	return dnc_read_status(status, s); // its synchronization also keeps the plan alive until the copy of its table has run
}

template int self_adjoint_evd_dev<double>(MatV<const double>, MatV<double>, double *, idx_t, idx_t, idx_t);
template int self_adjoint_evd_dev<float>(MatV<const float>, MatV<float>, float *, idx_t, idx_t, idx_t);

} // namespace fh
