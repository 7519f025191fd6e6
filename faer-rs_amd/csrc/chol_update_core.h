// Bodies of the Cholesky update kernels (chol_update.hip), written once for the device and for a host compiler.
//
// Restated from the reference: RankRUpdate::run of cholesky/llt/update.rs:271-345 and cholesky/ldlt/update.rs:244-320, real scalars.
// For column j and column k of W, with d = L[j, j] and p = W[j, k]:
//   LLT : nd = sqrt(d^2 + alpha_k p^2) (NonPositivePivot{j} if the radicand is <= 0; a NaN passes), gamma = nd / d,
//         beta = alpha_k p / nd, p' = -p / d, alpha_k -= beta^2
//   LDLT: nd = d + alpha_k p^2, beta = alpha_k p / nd, p' = -p, alpha_k -= nd beta^2 (d == 0 && nd == 0: beta = p' = 0, alpha_k kept)
//   rows i > j: w_ik = fma(p', l_ij, w_ik); l_ij = fma(beta, w_ik, gamma l_ij)   (gamma = 1 for LDLT)
// Step (j, k) reads what (j, k - 1) left in column j of L and what (j - 1, k) left in w_k and alpha_k, and nothing else: every
// order of the steps that respects these two edges gives the same bits.  The kernels walk a block of NB columns once per chunk of
// at most RC columns of W ("all j of the block, then the next chunk"), which is such an order.
//
// A "group" G owns the rows of one diagonal block: lane0() / lane1() is the range of rows the calling thread works on, lanes()
// their number over the whole group, sync() orders the group's accesses to the block's local memory.  On the device it is one
// wave with one row per lane; on the host (tests/host/chol_update_host.cpp) one thread that walks all rows, and sync() does nothing.
// Scalar decisions are taken by every lane redundantly from the same memory, so control flow is uniform.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define CU_HD __host__ __device__ inline
#define CU_UNROLL _Pragma("unroll")
#else
#define CU_HD inline
#define CU_UNROLL
#endif
// the coefficient formulas round every product and sum on its own, like the reference: contracting d * d + (alpha p) p into a fused
// multiply-add moves a downdate that cancels most of d (n = 1, r = 31: 70 -> 2) by tens of n eps
#ifdef __clang__
#define CU_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CU_NO_CONTRACT
#endif

namespace fh {
namespace cholup {

CU_HD double cu_sqrt(double x) { return sqrt(x); }
CU_HD float cu_sqrt(float x) { return sqrtf(x); }
CU_HD double cu_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
CU_HD float cu_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// the group of a host program: one thread that owns every row
struct HostGroup {
	int nlanes;
	int lane0() const { return 0; }
	int lane1() const { return nlanes; }
	int lanes() const { return nlanes; }
	void sync() const {}
};

// what the rows below column j need of step (j, k)
template <typename T> struct Coef {
	T pneg, beta, gamma;
};

// One step of the recurrence down the diagonal.  d: the pivot, replaced by the new one; dinv: 1 / d on entry and on return (LLT only:
// one division per step, the reciprocal of the new pivot serves the next k); alpha: alpha_k, updated.  false: non positive pivot.
template <bool LDLT, typename T> CU_HD bool coef_step(T &d, T &dinv, T p, T &alpha, Coef<T> &c)
{
	CU_NO_CONTRACT
	const T ap = alpha * p;
	if (LDLT) {
		const T nd = d + ap * p;
		if (d == 0 && nd == 0) {
			c.beta = 0;
			c.pneg = -(T) 0;
		} else {
			c.beta = ap * ((T) 1 / nd);
			alpha = alpha - nd * (c.beta * c.beta);
			c.pneg = -p;
		}
		c.gamma = 1;
		d = nd;
		return true;
	}
	const T nd2 = d * d + ap * p;
	if (nd2 <= 0)
		return false;
	const T nd = cu_sqrt(nd2);
	const T ndinv = (T) 1 / nd;
	c.gamma = nd * dinv;
	c.beta = ap * ndinv;
	c.pneg = -(p * dinv);
	alpha = alpha - c.beta * c.beta;
	d = nd;
	dinv = ndinv;
	return true;
}

// one entry of L and of W below the diagonal
template <bool LDLT, typename T> CU_HD void row_step(T &l, T &w, const Coef<T> &c)
{
	w = cu_fma(c.pneg, l, w);
	l = LDLT ? cu_fma(c.beta, w, l) : cu_fma(c.beta, w, c.gamma * l);
}

// The status word of a call is 0, or the smallest failing column + 1.  Columns of the block [j0, j0 + nb) a diagonal step still
// runs: all of them, or after a failure those in front of it (a later chunk of W may fail at a smaller column, and that is the
// column the reference reports).
CU_HD int diag_limit(int status, int j0, int nb)
{
	if (status == 0)
		return nb;
	const int l = status - 1 - j0;
	return l <= 0 ? 0 : (l > nb ? nb : l);
}

// Local memory of one diagonal block (LDS on the device): the lower triangle of the block column major, the chunk of W and the
// coefficients of the running column k major, the new diagonal, alpha_k before and after the running column.
template <typename T, int NB, int RC> struct DiagLocal {
	T l[NB * NB];
	T w[RC * NB];
	T dn[NB];
	T al[2][RC];
};

// The diagonal block of columns [j0, j0 + nb) against columns [0, rc) of W (rc <= RC; L, W and alpha point at the block's first row
// and the chunk's first column).  Reads and writes the lower triangle of the block, rows [0, nb) of the chunk and alpha; writes
// the coefficient table tab[jj * rc + k].  `limit`: columns of the block to run (< nb after a failure in an earlier chunk).
// Returns the columns completed: less than `limit` means that column failed (LLT); L then holds the completed columns, W and
// alpha are unspecified.
template <bool LDLT, int NB, int RC, typename T, typename G>
CU_HD int diag_block(const G &g, DiagLocal<T, NB, RC> &m, T *L, long lrs, long lcs, T *W, long wrs, long wcs, T *alpha, int nb, int rc, int limit, Coef<T> *tab)
{
	const int t0 = g.lane0(), t1 = g.lane1();
	for (int i = t0; i < t1; ++i) {
		if (i < nb) {
			for (int c = 0; c <= i; ++c)
				m.l[c * NB + i] = L[i * lrs + c * lcs];
			for (int k = 0; k < rc; ++k)
				m.w[k * NB + i] = W[i * wrs + k * wcs];
		}
		for (int k = i; k < rc; k += g.lanes())
			m.al[0][k] = alpha[k];
	}
	int done = limit;
	for (int jj = 0; jj < limit; ++jj) {
		g.sync(); // column jj - 1 wrote row jj of the block, its entries of W and alpha
		const T d0 = m.l[jj * NB + jj];
		const T *ain = m.al[jj & 1];
		T *aout = m.al[(jj + 1) & 1];
		bool ok = true;
		for (int i = t0; i < t1; ++i) {
			T d = d0, dinv = LDLT ? (T) 1 : (T) 1 / d0;
			const bool below = i > jj && i < nb;
			T l = below ? m.l[jj * NB + i] : (T) 0;
			for (int k = 0; k < rc; ++k) {
				T a = ain[k];
				Coef<T> c;
				ok = coef_step<LDLT, T>(d, dinv, m.w[k * NB + jj], a, c);
				if (!ok)
					break;
				if (i == 0) {
					tab[jj * rc + k] = c;
					aout[k] = a;
				}
				if (below) {
					T w = m.w[k * NB + i];
					row_step<LDLT, T>(l, w, c);
					m.w[k * NB + i] = w;
				}
			}
			if (!ok)
				break;
			if (i == jj)
				m.dn[jj] = d;
			if (below)
				m.l[jj * NB + i] = l;
		}
		if (!ok) { // every lane saw the same pivot
			done = jj;
			break;
		}
	}
	// (after a failure too: the columns in front of it are complete, and a later chunk runs them again from memory)
	g.sync();
	for (int i = t0; i < t1; ++i) {
		if (i < nb) {
			for (int c = 0; c <= i; ++c)
				L[i * lrs + c * lcs] = c == i && i < done ? m.dn[i] : m.l[c * NB + i];
			for (int k = 0; k < rc; ++k)
				W[i * wrs + k * wcs] = m.w[k * NB + i];
		}
		for (int k = i; k < rc; k += g.lanes())
			alpha[k] = m.al[done & 1][k];
	}
	return done;
}

// One row below the block: lrow = &L[i, j0], wrow = &W[i, k0]; tab as diag_block left it (any memory).  At most RCW (>= rc) entries of
// the row of W live in registers; the NB columns are walked in groups of U loads.
template <bool LDLT, int RCW, typename T> CU_HD void tail_row(T *lrow, long lcs, T *wrow, long wcs, int nb, int rc, const Coef<T> *tab)
{
	constexpr int U = 8;
	T w[RCW];
CU_UNROLL
	for (int k = 0; k < RCW; ++k)
		w[k] = k < rc ? wrow[k * wcs] : (T) 0;
	int jj = 0;
	for (; jj + U <= nb; jj += U) {
		T l[U];
CU_UNROLL
		for (int u = 0; u < U; ++u)
			l[u] = lrow[(jj + u) * lcs];
CU_UNROLL
		for (int u = 0; u < U; ++u) {
CU_UNROLL
			for (int k = 0; k < RCW; ++k)
				if (k < rc)
					row_step<LDLT, T>(l[u], w[k], tab[(jj + u) * rc + k]);
		}
CU_UNROLL
		for (int u = 0; u < U; ++u)
			lrow[(jj + u) * lcs] = l[u];
	}
	for (; jj < nb; ++jj) {
		T l = lrow[jj * lcs];
CU_UNROLL
		for (int k = 0; k < RCW; ++k)
			if (k < rc)
				row_step<LDLT, T>(l, w[k], tab[jj * rc + k]);
		lrow[jj * lcs] = l;
	}
CU_UNROLL
	for (int k = 0; k < RCW; ++k)
		if (k < rc)
			wrow[k * wcs] = w[k];
}

// ---- deletion (cholesky/ldlt/update.rs:417-461): pure index logic
// old index of row / column q of the matrix with the sorted `idx` removed
CU_HD long kept_index(long q, const long *idx, long r)
{
	long k = 0;
	while (k < r && idx[k] - k <= q)
		++k;
	return q + k;
}

} // namespace cholup
} // namespace fh
