// Arithmetic of the leaf of the complex triangular inverse (ctrtri.hip), written once for the device and for a host compiler
// (tests/host/ctrtri_host.cpp).  Complex values travel as (re, im) pairs of the real type R, so the header needs no HIP type.
//
// A leaf is an E x E lower-triangular block (identity padded past the matrix), held as two planes re / im, element (i, j) at
// plane[j * ld + i].  It is inverted in two stages:
//   substitution : each SB x SB diagonal sub-block, one column of the inverse at a time (ct_column): w_j = inv_j,
//                  w_i = -(sum_{j <= k < i} t_ik w_k) inv_i for i > j, with inv_i the reciprocal of t_ii -- computed once per diagonal
//                  entry (ct_recip) as conj(z) / |z|^2, unscaled, the form the complex solve and the complex LU of the library use;
//   doubling     : for pairs of s-wide diagonal blocks, s = SB, 2 SB, ..., E / 2:  W10 = -W11 (T10 W00)
//                  (faer/src/linalg/triangular_inverse.rs:43-123 with the solve written as a product with the inverse already at hand).
// The device runs the doubling products on the MFMA pipe; ct_leaf_host below is the same schedule in plain loops.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define CT_HD __host__ __device__ inline
#else
#define CT_HD inline
#endif
#ifdef __clang__
#define CT_UNROLL _Pragma("unroll")
#else
#define CT_UNROLL
#endif

namespace fh {
namespace ctrtri {

constexpr int E = 64;  // edge of a leaf
constexpr int SB = 16; // edge of a sub-block inverted by substitution

// inv = conj(p) / |p|^2   (p == 0 follows IEEE: NaNs)
template <typename R> CT_HD void ct_recip(R pr, R pi, R &ir, R &ii)
{
	const R den = pr * pr + pi * pi;
	ir = pr / den;
	ii = -pi / den;
}

// acc += a * b
template <typename R> CT_HD void ct_mac(R &sr, R &si, R ar, R ai, R br, R bi)
{
	sr += ar * br - ai * bi;
	si += ar * bi + ai * br;
}

// Column j of the inverse of the SB x SB lower-triangular sub-block whose (0, 0) is at tre / tim (leading dimension ld): wr / wi [SB],
// zeros above row j.  ivr / ivi [SB] are the reciprocals of the sub-block's diagonal ((1, 0) for a unit diagonal: the diagonal
// of t is not read here).
template <typename R> CT_HD void ct_column(const R *tre, const R *tim, int ld, const R *ivr, const R *ivi, int j, R *wr, R *wi)
{
	CT_UNROLL
	for (int i = 0; i < SB; ++i) {
		R sr = (R) 0, si = (R) 0;
		CT_UNROLL
		for (int k = 0; k < i; ++k)
			if (k >= j)
				ct_mac(sr, si, tre[k * ld + i], tim[k * ld + i], wr[k], wi[k]);
		R xr = (R) 0, xi = (R) 0;
		if (i == j) {
			xr = ivr[i];
			xi = ivi[i];
		} else if (i > j) {
			ct_mac(xr, xi, -sr, -si, ivr[i], ivi[i]);
		}
		wr[i] = xr;
		wi[i] = xi;
	}
}

// The whole leaf on one thread: re / im (E x E planes, leading dimension ld, lower triangle valid, identity padded) become the
// inverse's lower triangle.  tr / ti: E * E / 4 reals of workspace each.  The host program's leaf; the device leaf splits the
// same stages over its threads.
template <typename R> inline void ct_leaf_host(R *re, R *im, int ld, bool unit, R *tr, R *ti)
{
	R ivr[E], ivi[E];
	for (int d = 0; d < E; ++d) {
		ivr[d] = (R) 1;
		ivi[d] = (R) 0;
		if (!unit)
			ct_recip(re[d * ld + d], im[d * ld + d], ivr[d], ivi[d]);
	}
	for (int c0 = 0; c0 < E; c0 += SB) {
		R wr[SB][SB], wi[SB][SB];
		for (int j = 0; j < SB; ++j)
			ct_column(re + c0 * ld + c0, im + c0 * ld + c0, ld, ivr + c0, ivi + c0, j, wr[j], wi[j]);
		for (int j = 0; j < SB; ++j)
			for (int i = j; i < SB; ++i) {
				re[(c0 + j) * ld + c0 + i] = wr[j][i];
				im[(c0 + j) * ld + c0 + i] = wi[j][i];
			}
	}
	for (int s = SB; s < E; s *= 2)
		for (int c = 0; c < E; c += 2 * s) {
			// P = T10 W00 (s x s, column major in tr / ti), then W10 = -W11 P
			for (int j = 0; j < s; ++j)
				for (int i = 0; i < s; ++i) {
					R sr = (R) 0, si = (R) 0;
					for (int k = j; k < s; ++k)
						ct_mac(sr, si, re[(c + k) * ld + c + s + i], im[(c + k) * ld + c + s + i], re[(c + j) * ld + c + k],
						       im[(c + j) * ld + c + k]);
					tr[j * s + i] = sr;
					ti[j * s + i] = si;
				}
			for (int j = 0; j < s; ++j)
				for (int i = 0; i < s; ++i) {
					R sr = (R) 0, si = (R) 0;
					for (int k = 0; k <= i; ++k)
						ct_mac(sr, si, re[(c + s + k) * ld + c + s + i], im[(c + s + k) * ld + c + s + i], tr[j * s + k], ti[j * s + k]);
					re[(c + j) * ld + c + s + i] = -sr;
					im[(c + j) * ld + c + s + i] = -si;
				}
		}
}

} // namespace ctrtri
} // namespace fh
