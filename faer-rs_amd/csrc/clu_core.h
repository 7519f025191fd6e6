// Arithmetic of one elimination step of the complex partial-pivot LU (cgetrf.hip), written once for the device and for a host compiler
// (tests/host/clu_host.cpp).  Complex values travel as (re, im) pairs of the real type R, so the header needs no HIP type.
//
// Restated from the reference (lu/partial_pivoting/factor.rs:19-67), for column j of a panel:
//   pivot search : the first row i >= j whose abs1 = |re| + |im| is strictly larger than every earlier candidate's, starting from 0
//                  -- an all-zero column keeps row j, a NaN is never chosen (both comparisons with a NaN are false);
//   reciprocal   : inv = conj(p) / |p|^2, unscaled (|p|^2 may overflow or underflow; p == 0 gives NaNs: 0 / 0);
//   scaling      : l_i = a_ij * inv for the rows below the pivot;
//   update       : a_ic -= l_i * u_c for the columns right of j.
// A search split over lanes, waves and workgroups keeps the reference's answer through clu_better(): among candidates of equal abs1
// the smaller row wins, which is the row a single ascending scan would have met first.  The rule is a strict order on distinct
// (value, row) pairs, so a reduction in any shape ends with the same pair.
// Every product and sum rounds on its own (no fused multiply-add): the host restatement in tests/complex_lu_ref.py does the same.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define CLU_HD __host__ __device__ inline
#else
#define CLU_HD inline
#endif
#ifdef __clang__
#define CLU_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CLU_NO_CONTRACT
#endif

namespace fh {
namespace clu {

CLU_HD double clu_fabs(double x) { return fabs(x); }
CLU_HD float clu_fabs(float x) { return fabsf(x); }

template <typename R> CLU_HD R clu_abs1(R re, R im) { return clu_fabs(re) + clu_fabs(im); }

// does the candidate (v, row) replace the current best (bv, brow)?  The search starts from (0, j).
template <typename R> CLU_HD bool clu_better(R v, int row, R bv, int brow) { return v > bv || (v == bv && row < brow); }

template <typename R> CLU_HD void clu_consider(R v, int row, R &bv, int &brow)
{
	if (clu_better(v, row, bv, brow)) {
		bv = v;
		brow = row;
	}
}

// inv = conj(p) / |p|^2
template <typename R> CLU_HD void clu_recip(R pr, R pi, R &ir, R &ii)
{
	CLU_NO_CONTRACT
	const R den = pr * pr + pi * pi;
	ir = pr / den;
	ii = -pi / den;
}

// l = a * inv
template <typename R> CLU_HD void clu_scale(R ar, R ai, R ir, R ii, R &lr, R &li)
{
	CLU_NO_CONTRACT
	lr = ar * ir - ai * ii;
	li = ar * ii + ai * ir;
}

// x -= l * u
template <typename R> CLU_HD void clu_update(R &xr, R &xi, R lr, R li, R ur, R ui)
{
	CLU_NO_CONTRACT
	xr -= lr * ur - li * ui;
	xi -= lr * ui + li * ur;
}

// The whole factorization with these bodies, one thread: a (m x n, column major planes re / im with leading dimension m) becomes
// unit-lower L and U in place, piv[j] = the row exchanged with row j, j < min(m, n).  The host program's driver; the device panels
// run the same steps split over their threads.
template <typename R> inline void clu_factor_unblocked(int m, int n, R *re, R *im, int *piv)
{
	const int k = m < n ? m : n;
	for (int j = 0; j < k; ++j) {
		R bv = (R) 0;
		int p = j;
		for (int i = j; i < m; ++i)
			clu_consider(clu_abs1(re[j * m + i], im[j * m + i]), i, bv, p);
		piv[j] = p;
		if (p != j)
			for (int c = 0; c < n; ++c) {
				R t = re[c * m + j];
				re[c * m + j] = re[c * m + p];
				re[c * m + p] = t;
				t = im[c * m + j];
				im[c * m + j] = im[c * m + p];
				im[c * m + p] = t;
			}
		R ir, ii;
		clu_recip(re[j * m + j], im[j * m + j], ir, ii);
		for (int i = j + 1; i < m; ++i) {
			R lr, li;
			clu_scale(re[j * m + i], im[j * m + i], ir, ii, lr, li);
			re[j * m + i] = lr;
			im[j * m + i] = li;
			for (int c = j + 1; c < n; ++c)
				clu_update(re[c * m + i], im[c * m + i], lr, li, re[c * m + j], im[c * m + j]);
		}
	}
}

} // namespace clu
} // namespace fh
