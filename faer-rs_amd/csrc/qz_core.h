// Bodies of the generalized real eigendecomposition (qz.hip), written once for the device and for a host compiler, against the
// group abstraction of schur_core.h (tid(), size(), sync()): tests/host/qz_host.cpp runs them on one thread.
//
// Every transformation is a plane rotation of two rows or two columns, applied by all threads of the group across H, T and
// the orthogonal factor in one pass.  The scalars of a rotation are read by every thread from the same memory (ldc), so control
// flow is uniform; the entries a rotation sets exactly (its r and its 0) are stored by thread 0 in the same pass, outside the
// ranges the other threads rotate.  Between threads the rule is read, sync, store, sync.
//
// Restated from the reference: generalized_hessenberg_unblocked (gevd/gen_hessenberg/mod.rs:82-155), hessenberg_to_qz_unblocked
// with single_shift_sweep / double_shift_sweep (gevd/qz_real/mod.rs:475-1420; LAPACK's hgeqz) and qz_to_gevd_real
// (gevd/mod.rs:491-1005; LAPACK's tgevc).  Deviations are listed in DESIGN.md 3.14.
#pragma once
#include "schur_core.h"

namespace fh {
namespace qz {

using namespace schur;

// counters of one call (ints): what the host reads back once
enum { QC_STATUS = 0, QC_SWEEPS = 1, QC_INFINITE = 2, QC_NONFINITE = 3, QC_COUNT = 16 };

// (c, s, r) with [c s; -s c] (f, g)^T = (r, 0)^T
template <typename T> SC_HD void givens(T f, T g, T &c, T &s, T &r)
{
	if (g == 0) {
		c = 1;
		s = 0;
		r = f;
		return;
	}
	r = sc_hypot(f, g);
	c = f / r;
	s = g / r;
}

// n pairs (x[k step], x[k step + dy])
template <typename T> struct Seg {
	T *x;
	long dy, step, n;
};

// (x, y) <- (c x + s y, c y - s x) on every pair of the three segments; thread 0 stores rv to *rp and 0 to *zp (a pair the
// segments leave out) in the same pass
template <typename T, typename G> SC_HD void rot3(const G &g, Seg<T> a, Seg<T> b, Seg<T> c, T cs, T sn, T *rp, T rv, T *zp)
{
	if (a.n < 0 || !a.x)
		a.n = 0;
	if (b.n < 0 || !b.x)
		b.n = 0;
	if (c.n < 0 || !c.x)
		c.n = 0;
	g.sync();
	const long total = a.n + b.n + c.n;
	for (long w = g.tid(); w < total; w += g.size()) {
		T *x;
		long dy;
		if (w < a.n) {
			x = a.x + w * a.step;
			dy = a.dy;
		} else if (w < a.n + b.n) {
			x = b.x + (w - a.n) * b.step;
			dy = b.dy;
		} else {
			x = c.x + (w - a.n - b.n) * c.step;
			dy = c.dy;
		}
		const T xv = x[0], yv = x[dy];
		x[0] = cs * xv + sn * yv;
		x[dy] = cs * yv - sn * xv;
	}
	if (g.tid() == 0 && rp) {
		*rp = rv;
		*zp = 0;
	}
	g.sync();
}

template <typename T, typename G> SC_HD void set_entry(const G &g, T *p, T v)
{
	g.sync();
	if (g.tid() == 0)
		*p = v;
	g.sync();
}

// the pair (H, T), n x n column major, and its two orthogonal factors (nullptr: not accumulated)
template <typename T> struct Pencil {
	T *h;
	long ldh;
	T *t;
	long ldt;
	long n;
	T *q;
	long ldq;
	T *z;
	long ldz;
	SC_HD T *H(long i, long j) const { return h + i + j * ldh; }
	SC_HD T *B(long i, long j) const { return t + i + j * ldt; }
};

// rows i, i + 1 of H from column hc0 and of T from column tc0; columns i, i + 1 of Q
template <typename T, typename G> SC_HD void left_rot(const G &g, const Pencil<T> &p, long i, T c, T s, long hc0, long tc0, T *rp, T rv, T *zp)
{
	if (hc0 < 0)
		hc0 = 0;
	rot3(g, Seg<T>{p.H(i, hc0), 1, p.ldh, p.n - hc0}, Seg<T>{p.B(i, tc0), 1, p.ldt, p.n - tc0},
	     Seg<T>{p.q ? p.q + i * p.ldq : nullptr, p.ldq, 1, p.n}, c, s, rp, rv, zp);
}
// columns j, j + 1 of H in rows [0, hr1) and of T in rows [0, tr1); columns j, j + 1 of Z
template <typename T, typename G> SC_HD void right_rot(const G &g, const Pencil<T> &p, long j, T c, T s, long hr1, long tr1, T *rp, T rv, T *zp)
{
	rot3(g, Seg<T>{p.H(0, j), p.ldh, 1, hr1}, Seg<T>{p.B(0, j), p.ldt, 1, tr1}, Seg<T>{p.z ? p.z + j * p.ldz : nullptr, p.ldz, 1, p.n}, c, s,
	     rp, rv, zp);
}
// the rotation of columns j, j + 1 that puts x (column j) into y (column j + 1): (x, y) -> (0, r)
template <typename T> SC_HD void givens_right(T x, T y, T &c, T &s, T &r)
{
	T cc, ss;
	givens(y, x, cc, ss, r);
	c = cc;
	s = -ss;
}
// column j of H (rows [0, hr1)), T (rows [0, tr1)) and Z changes sign
template <typename T, typename G> SC_HD void negate_col(const G &g, const Pencil<T> &p, long j, long hr1, long tr1)
{
	g.sync();
	const long nz = p.z ? p.n : 0;
	for (long w = g.tid(); w < hr1 + tr1 + nz; w += g.size()) {
		T *x = w < hr1 ? p.H(w, j) : (w < hr1 + tr1 ? p.B(w - hr1, j) : p.z + (w - hr1 - tr1) + j * p.ldz);
		*x = -*x;
	}
	g.sync();
}

// gen_hessenberg/mod.rs:82-155: (A, B), B upper triangular -> (Hessenberg, triangular); Q <- Q G^T, Z <- Z G^T
template <typename T, typename G> SC_HD void hessenberg_triangular(const G &g, const Pencil<T> &p)
{
	const long n = p.n;
	for (long jcol = 0; jcol + 2 < n; ++jcol)
		for (long i = n - 1; i >= jcol + 2; --i) {
			T c, s, r;
			g.sync();
			givens(ldc(p.H(i - 1, jcol)), ldc(p.H(i, jcol)), c, s, r);
			left_rot(g, p, i - 1, c, s, jcol + 1, i - 1, p.H(i - 1, jcol), r, p.H(i, jcol));
			givens_right(ldc(p.B(i, i - 1)), ldc(p.B(i, i)), c, s, r);
			right_rot(g, p, i - 1, c, s, n, i, p.B(i, i), r, p.B(i, i - 1));
		}
}

// Eigenvalues w (sa / sb) of the 2 x 2 pencil (a, b), b upper triangular with a nonzero diagonal: real (wi == 0): w1, w2;
// a conjugate pair: w1 +- i wi.  (The role of lag2, qz_real/mod.rs.)
template <typename T> SC_HD void lag2(T a11, T a12, T a21, T a22, T b11, T b12, T b22, T &sa, T &sb, T &w1, T &w2, T &wi)
{
	const T tiny = Lim<T>::tiny();
	sa = sc_max(sc_max(sc_abs(a11), sc_abs(a12)), sc_max(sc_max(sc_abs(a21), sc_abs(a22)), tiny));
	sb = sc_max(sc_max(sc_abs(b11), sc_abs(b12)), sc_max(sc_abs(b22), tiny));
	a11 /= sa;
	a12 /= sa;
	a21 /= sa;
	a22 /= sa;
	b11 /= sb;
	b12 /= sb;
	b22 /= sb;
	if (sc_abs(b11) < tiny)
		b11 = tiny;
	if (sc_abs(b22) < tiny)
		b22 = tiny;
	const T k11 = a11 / b11, k21 = a21 / b11, k12 = (a12 - k11 * b12) / b22, k22 = (a22 - k21 * b12) / b22;
	const T m = (k11 + k22) * (T) 0.5, hd = (k11 - k22) * (T) 0.5;
	const T sc = sc_max(sc_max(sc_abs(hd), sc_abs(k12)), sc_max(sc_abs(k21), tiny));
	const T d = (hd / sc) * (hd / sc) + (k12 / sc) * (k21 / sc);
	if (d >= 0) {
		const T rt = sc * sc_sqrt(d);
		w1 = m + rt;
		w2 = m - rt;
		wi = 0;
	} else {
		w1 = w2 = m;
		wi = sc * sc_sqrt(-d);
	}
}

// one step of a chase: the rotation of rows j, j + 1 that was prepared (c, s) or that clears H(j + 1, j - 1), then the rotation
// of columns j, j + 1 that restores T(j + 1, j) = 0
template <typename T, typename G> SC_HD void single_step(const G &g, const Pencil<T> &p, long j, long ilast, bool from_column, T c, T s)
{
	T r = 0;
	g.sync();
	if (from_column)
		givens(ldc(p.H(j, j - 1)), ldc(p.H(j + 1, j - 1)), c, s, r);
	left_rot(g, p, j, c, s, j, j, from_column ? p.H(j, j - 1) : (T *) nullptr, r, from_column ? p.H(j + 1, j - 1) : (T *) nullptr);
	givens_right(ldc(p.B(j + 1, j)), ldc(p.B(j + 1, j + 1)), c, s, r);
	right_rot(g, p, j, c, s, sc_min(j + 3, ilast + 1), j + 1, p.B(j + 1, j + 1), r, p.B(j + 1, j));
}

// first column of (K - s1)(K - s2), K = (H / sa) (T / sb)^-1, from the leading 3 x 2 of K at row f0; tr = s1 + s2, det = s1 s2
template <typename T> SC_HD void shift_vector(const Pencil<T> &p, long f0, T tr, T det, T sa, T sb, T &v1, T &v2, T &v3)
{
	const long f1 = f0 + 1;
	const T t00 = ldc(p.B(f0, f0)) / sb, t01 = ldc(p.B(f0, f1)) / sb, t11 = ldc(p.B(f1, f1)) / sb;
	const T k11 = (ldc(p.H(f0, f0)) / sa) / t00, k21 = (ldc(p.H(f1, f0)) / sa) / t00;
	const T k12 = (ldc(p.H(f0, f1)) / sa - k11 * t01) / t11, k22 = (ldc(p.H(f1, f1)) / sa - k21 * t01) / t11;
	const T k32 = (ldc(p.H(f1 + 1, f1)) / sa) / t11;
	v1 = k11 * k11 + k12 * k21 - tr * k11 + det;
	v2 = k21 * (k11 + k22 - tr);
	v3 = k21 * k32;
}

// One step of a double-shift chase on rows j .. j + 2: the 3-vector (v, or column j - 1 of H when col) is cleared by two row
// rotations (which leave T(j + 2, j) zero), then two column rotations restore T.  ilast: last row of the active block.
template <typename T, typename G> SC_HD void double_step(const G &g, const Pencil<T> &p, long j, long ilast, bool col, T v1, T v2, T v3)
{
	g.sync();
	if (col) {
		v1 = ldc(p.H(j, j - 1));
		v2 = ldc(p.H(j + 1, j - 1));
		v3 = ldc(p.H(j + 2, j - 1));
	}
	T c, s, r1, r2, r;
	givens(v2, v3, c, s, r1);
	left_rot(g, p, j + 1, c, s, j, j + 1, col ? p.H(j + 1, j - 1) : (T *) nullptr, r1, col ? p.H(j + 2, j - 1) : (T *) nullptr);
	givens(v1, r1, c, s, r2);
	left_rot(g, p, j, c, s, j, j, col ? p.H(j, j - 1) : (T *) nullptr, r2, col ? p.H(j + 1, j - 1) : (T *) nullptr);
	givens_right(ldc(p.B(j + 2, j + 1)), ldc(p.B(j + 2, j + 2)), c, s, r);
	right_rot(g, p, j + 1, c, s, sc_min(j + 4, ilast + 1), j + 2, p.B(j + 2, j + 2), r, p.B(j + 2, j + 1));
	givens_right(ldc(p.B(j + 1, j)), ldc(p.B(j + 1, j + 1)), c, s, r);
	right_rot(g, p, j, c, s, sc_min(j + 4, ilast + 1), j + 1, p.B(j + 1, j + 1), r, p.B(j + 1, j));
}

// One window step of a multishift sweep (the counterpart of schur_core.h's window_chase, same geometry): p is the ws x ws window
// of (H, T) at global row w0 with its two accumulators (identities on entry).  Bulge b of nb uses the shifts (sr, si)[2 b],
// [2 b + 1] and takes the steps whose column index k (global) runs over [A - 3 b, B - 3 b), clipped to [ilo - 1, ihi - 2):
// k == ilo - 1 introduces it at the top of the active block [ilo, ihi), the last two rows let it run off.  The shifts are
// eigenvalues of (H / sa, T / sb), sa = |H|_F, sb = |T|_F of the whole pair (qz_sweep_shifts), and the first column of the bulge
// is formed in those units: of order one whatever the scales of A and B, and unchanged when either is scaled by a power of two.
template <typename T, typename G>
SC_HD void qz_window_chase(const G &g, const Pencil<T> &p, long w0, long ilo, long ihi, int nb, const T *sr, const T *si, T sa, T sb, long A, long B)
{
	const long ilast = sc_min(ihi - w0, p.n) - 1;
	for (int b = 0; b < nb; ++b) {
		long ka = A - 3 * b, kb = B - 3 * b;
		if (ka < ilo - 1)
			ka = ilo - 1;
		if (kb > ihi - 2)
			kb = ihi - 2;
		const T s1r = sr[2 * b], s1i = si[2 * b], s2r = sr[2 * b + 1], s2i = si[2 * b + 1];
		for (long k = ka; k < kb; ++k) {
			const long j = k + 1 - w0, left = ihi - (k + 1);
			const bool intro = k == ilo - 1;
			if (left >= 3) {
				T v1 = 0, v2 = 0, v3 = 0;
				g.sync();
				if (intro)
					shift_vector(p, j, s1r + s2r, s1r * s2r - s1i * s2i, sa, sb, v1, v2, v3);
				double_step(g, p, j, ilast, !intro, v1, v2, v3);
			} else {
				single_step(g, p, j, ilast, true, (T) 1, (T) 0);
			}
		}
	}
	g.sync();
}

// (the same in the units of H and T themselves, sa = sb = 1, for a pair near unit scale: a host program that holds no norms)
template <typename T, typename G>
SC_HD void qz_window_chase(const G &g, const Pencil<T> &p, long w0, long ilo, long ihi, int nb, const T *sr, const T *si, long A, long B)
{
	qz_window_chase(g, p, w0, ilo, ihi, nb, sr, si, (T) 1, (T) 1, A, B);
}

// The ns shifts of a sweep on the block that ends at row istop (exclusive) of the n x n pair (h, t) in global memory: the
// eigenvalues ((ar + i ai) / sa) / (be / sb) of its trailing ns x ns sub-pencil in units of sa = |H|_F, sb = |T|_F, that is the
// eigenvalues of (H / sa, T / sb) (err != 0: they are not all there), paired as schur_core.h pairs them.  An infinite or missing
// eigenvalue, or `exceptional`, gives the ad hoc shifts h(i, i - 1) / t(i - 1, i - 1) + h(i, i) / t(i, i) of the trailing rows
// in the same units.  No quotient of an entry of H by an entry of T is formed unscaled: lambda itself need not be representable.
// One thread.
template <typename T>
SC_HD void qz_sweep_shifts(const T *h, long ldh, const T *t, long ldt, long istop, int ns, bool exceptional, long err, const T *ar, const T *ai, const T *be,
			   T sa, T sb, T *wr, T *wi)
{
	bool bad = exceptional || err != 0;
	for (int i = 0; i < ns && !bad; ++i)
		bad = be[i] == 0;
	for (int i = 0; i < ns; ++i) {
		const long r = istop - ns + i;
		if (bad) {
			wr[i] = (h[r + (r - 1) * ldh] / sa) / (t[(r - 1) + (r - 1) * ldt] / sb) + (h[r + r * ldh] / sa) / (t[r + r * ldt] / sb);
			wi[i] = 0;
		} else {
			wr[i] = (ar[i] / sa) / (be[i] / sb);
			wi[i] = (ai[i] / sa) / (be[i] / sb);
		}
	}
	const long e = istop - 1;
	pair_shifts(wr, wi, ns, (h[e + e * ldh] / sa) / (t[e + e * ldt] / sb));
}

// (in the units of H and T themselves, to go with the window chase in those units)
template <typename T>
SC_HD void qz_sweep_shifts(const T *h, long ldh, const T *t, long ldt, long istop, int ns, bool exceptional, long err, const T *ar, const T *ai, const T *be,
			   T *wr, T *wi)
{
	qz_sweep_shifts(h, ldh, t, ldt, istop, ns, exceptional, err, ar, ai, be, (T) 1, (T) 1, wr, wi);
}

// The QZ iteration on the Hessenberg-triangular pair p (the whole matrix is the active block): on return H is quasi upper
// triangular, T upper triangular, every 2 x 2 block of H belongs to a conjugate pair and has a diagonal block of T with positive
// entries; (ar + i ai) / be are the eigenvalues, be >= 0, be == 0 exactly for the infinite ones a negligible diagonal entry of T
// gave.  anorm / bnorm: Frobenius norms of H and T.  cap: most iterations (30 max(10, n) in the drivers).  cnt: QC_SWEEPS and
// QC_INFINITE are counted up.  Returns 0, or the number of eigenvalues not found when the cap is reached.
// Scan mode (min_return > 0; the prepare step of the driver): the iteration starts at row ilast0 and returns -1 with
// [bfirst, blast] as soon as the active block has min_return rows or more; smaller blocks are finished in place.
template <typename T, typename G>
SC_HD long qz_unblocked(const G &g, const Pencil<T> &p, T *ar, T *ai, T *be, T anorm, T bnorm, long cap, int *cnt, long ilast0, long min_return,
			long &bfirst, long &blast)
{
	const int t = g.tid();
	const long n = p.n;
	const T ulp = Lim<T>::eps(), safmin = Lim<T>::tiny();
	const T atol = sc_max(safmin, ulp * anorm), btol = sc_max(safmin, ulp * bnorm);
	const T ascale = 1 / sc_max(safmin, anorm);
	long ilast = ilast0, iiter = 0;
	T eshift = 0;
	(void) n;
	for (long jiter = 0; ilast >= 0; ++jiter) {
		if (jiter >= cap)
			return ilast + 1;
		g.sync();
		long ifirst = -1;
		int action = 0; // 0: a sweep on [ifirst, ilast]; 1: deflate row ilast; 2: T(ilast, ilast) == 0, clear H(ilast, ilast - 1) first
		if (ilast == 0) {
			if (sc_abs(ldc(p.B(0, 0))) <= btol)
				set_entry(g, p.B(0, 0), (T) 0);
			action = 1;
		} else if (sc_abs(ldc(p.H(ilast, ilast - 1))) <= atol) {
			set_entry(g, p.H(ilast, ilast - 1), (T) 0);
			action = 1;
		} else if (sc_abs(ldc(p.B(ilast, ilast))) <= btol) {
			set_entry(g, p.B(ilast, ilast), (T) 0);
			action = 2;
		} else {
			for (long j = ilast - 1; j >= 0; --j) {
				bool ilazro = j == 0;
				if (!ilazro && sc_abs(ldc(p.H(j, j - 1))) <= atol) {
					set_entry(g, p.H(j, j - 1), (T) 0);
					ilazro = true;
				}
				if (sc_abs(ldc(p.B(j, j))) < btol) { // (strict in the interior, <= at the bottom, as in the reference)
					set_entry(g, p.B(j, j), (T) 0);
					bool ilazr2 = false;
					if (!ilazro
					    && sc_abs(ldc(p.H(j, j - 1))) * (ascale * sc_abs(ldc(p.H(j + 1, j)))) <= sc_abs(ldc(p.H(j, j))) * (ascale * atol))
						ilazr2 = true;
					if (ilazro || ilazr2) {
						// the block splits at row j: rotate the zero of T down while the diagonal below is negligible too
						action = 2;
						for (long jch = j; jch < ilast; ++jch) {
							T c, s, r;
							g.sync();
							givens(ldc(p.H(jch, jch)), ldc(p.H(jch + 1, jch)), c, s, r);
							left_rot(g, p, jch, c, s, jch + 1, jch + 1, p.H(jch, jch), r, p.H(jch + 1, jch));
							if (ilazr2)
								set_entry(g, p.H(jch, jch - 1), ldc(p.H(jch, jch - 1)) * c);
							ilazr2 = false;
							if (sc_abs(ldc(p.B(jch + 1, jch + 1))) >= btol) {
								if (jch + 1 >= ilast)
									action = 1;
								else {
									ifirst = jch + 1;
									action = 0;
								}
								break;
							}
							set_entry(g, p.B(jch + 1, jch + 1), (T) 0);
						}
					} else {
						// T(j, j) == 0 inside an unreduced block: chase the zero to the bottom
						for (long jch = j; jch < ilast; ++jch) {
							T c, s, r;
							g.sync();
							givens(ldc(p.B(jch, jch + 1)), ldc(p.B(jch + 1, jch + 1)), c, s, r);
							left_rot(g, p, jch, c, s, jch - 1, jch + 2, p.B(jch, jch + 1), r, p.B(jch + 1, jch + 1));
							givens_right(ldc(p.H(jch + 1, jch - 1)), ldc(p.H(jch + 1, jch)), c, s, r);
							right_rot(g, p, jch - 1, c, s, jch + 1, jch, p.H(jch + 1, jch), r, p.H(jch + 1, jch - 1));
						}
						action = 2;
					}
					break;
				}
				if (ilazro) {
					ifirst = j;
					break;
				}
			}
		}
		if (action == 2) {
			T c, s, r;
			g.sync();
			givens_right(ldc(p.H(ilast, ilast - 1)), ldc(p.H(ilast, ilast)), c, s, r);
			right_rot(g, p, ilast - 1, c, s, ilast, ilast, p.H(ilast, ilast), r, p.H(ilast, ilast - 1));
			action = 1;
		}
		if (action == 1) {
			g.sync();
			if (ldc(p.B(ilast, ilast)) < 0)
				negate_col(g, p, ilast, ilast + 1, ilast + 1);
			g.sync();
			if (t == 0) {
				ar[ilast] = ldc(p.H(ilast, ilast));
				ai[ilast] = 0;
				be[ilast] = ldc(p.B(ilast, ilast));
				if (be[ilast] == 0)
					cnt[QC_INFINITE] += 1;
			}
			--ilast;
			iiter = 0;
			eshift = 0;
			continue;
		}
		if (min_return > 0 && ilast - ifirst + 1 >= min_return) {
			bfirst = ifirst;
			blast = ilast;
			return -1;
		}
		// ---- a sweep on the unreduced block [ifirst, ilast]
		++iiter;
		g.sync();
		const long l = ilast - 1;
		T wr = 0, sa = 1, sb = 1, w1 = 0, w2 = 0, wi = 0;
		bool single = true;
		if (iiter % 10 == 0) {
			eshift += ldc(p.H(ilast, l)) / ldc(p.B(l, l));
			wr = eshift;
		} else {
			lag2(ldc(p.H(l, l)), ldc(p.H(l, ilast)), ldc(p.H(ilast, l)), ldc(p.H(ilast, ilast)), ldc(p.B(l, l)), ldc(p.B(l, ilast)),
			     ldc(p.B(ilast, ilast)), sa, sb, w1, w2, wi);
			if (wi == 0) {
				const T hl = ldc(p.H(ilast, ilast)), tl = ldc(p.B(ilast, ilast));
				if (sc_abs(w1 * sa * (tl / sb) - hl) > sc_abs(w2 * sa * (tl / sb) - hl))
					w1 = w2;
				// the shift w1 of (H / sa, T / sb): the first column of the sweep is formed in those units, where no product
				// of a scale of H by a scale of T can leave the range
				wr = w1;
			} else
				single = false;
		}
		if (!single && ifirst + 1 == ilast) {
			// a 2 x 2 block with a conjugate pair: T <- its singular values (the role of svd_triu_2x2), then (alpha, beta)
			T f = ldc(p.B(l, l)), gq = ldc(p.B(l, ilast)), hh = ldc(p.B(ilast, ilast));
			const T sc = sc_max(sc_abs(f), sc_max(sc_abs(gq), sc_abs(hh)));
			f /= sc;
			gq /= sc;
			hh /= sc;
			const T gam = f * gq;
			T cr = 1, sr = 0;
			if (gam != 0) {
				const T zeta = (f * f - (gq * gq + hh * hh)) / (2 * gam);
				const T tt = (zeta >= 0 ? (T) 1 : (T) -1) / (sc_abs(zeta) + sc_sqrt(1 + zeta * zeta));
				cr = 1 / sc_sqrt(1 + tt * tt);
				sr = tt * cr;
			}
			right_rot(g, p, l, cr, sr, ilast + 1, ilast + 1, (T *) nullptr, (T) 0, (T *) nullptr);
			T cl, sl, r;
			givens(ldc(p.B(l, l)), ldc(p.B(ilast, l)), cl, sl, r);
			left_rot(g, p, l, cl, sl, l, ilast, p.B(l, l), r, p.B(ilast, l));
			set_entry(g, p.B(l, ilast), (T) 0);
			if (ldc(p.B(l, l)) < 0)
				negate_col(g, p, l, ilast + 1, l + 1);
			g.sync();
			if (ldc(p.B(ilast, ilast)) < 0)
				negate_col(g, p, ilast, ilast + 1, ilast + 1);
			g.sync();
			lag2(ldc(p.H(l, l)), ldc(p.H(l, ilast)), ldc(p.H(ilast, l)), ldc(p.H(ilast, ilast)), ldc(p.B(l, l)), (T) 0, ldc(p.B(ilast, ilast)), sa, sb,
			     w1, w2, wi);
			if (wi == 0)
				continue; // real after all: the single-shift sweeps of the next rounds split it
			const T mag = sc_abs(w1) + wi, fsc = mag > 1 ? 1 / mag : (T) 1;
			if (t == 0) {
				ar[l] = ar[ilast] = w1 * fsc * sa;
				ai[l] = wi * fsc * sa;
				ai[ilast] = -(wi * fsc * sa);
				be[l] = be[ilast] = sb * fsc;
			}
			ilast -= 2;
			iiter = 0;
			eshift = 0;
			continue;
		}
		if (t == 0)
			cnt[QC_SWEEPS] += 1;
		if (single) {
			T c, s, r;
			givens(ldc(p.H(ifirst, ifirst)) / sa - wr * (ldc(p.B(ifirst, ifirst)) / sb), ldc(p.H(ifirst + 1, ifirst)) / sa, c, s, r);
			for (long j = ifirst; j < ilast; ++j)
				single_step(g, p, j, ilast, j > ifirst, c, s);
			continue;
		}
		// double shift: first column of (K - w)(K - conj w), K = (H / sa) (T / sb)^-1
		T v1, v2, v3;
		shift_vector(p, ifirst, 2 * w1, w1 * w1 + wi * wi, sa, sb, v1, v2, v3);
		for (long j = ifirst; j + 2 <= ilast; ++j)
			double_step(g, p, j, ilast, j > ifirst, v1, v2, v3);
		single_step(g, p, ilast - 1, ilast, true, (T) 1, (T) 0);
	}
	return 0;
}

// ---- eigenvectors of the quasi-triangular pair

template <typename T> struct Cx {
	T r, i;
};
template <typename T> SC_HD Cx<T> cx_sub(Cx<T> a, Cx<T> b) { return Cx<T>{a.r - b.r, a.i - b.i}; }
template <typename T> SC_HD Cx<T> cx_mul(Cx<T> a, Cx<T> b) { return Cx<T>{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
template <typename T> SC_HD T cx_abs1(Cx<T> a) { return sc_abs(a.r) + sc_abs(a.i); }
template <typename T> SC_HD Cx<T> cx_div(Cx<T> a, Cx<T> b)
{
	if (sc_abs(b.r) >= sc_abs(b.i)) {
		const T e = b.i / b.r, f = b.r + b.i * e;
		return Cx<T>{(a.r + a.i * e) / f, (a.i - a.r * e) / f};
	}
	const T e = b.r / b.i, f = b.i + b.r * e;
	return Cx<T>{(a.r * e + a.i) / f, (a.i * e - a.r) / f};
}

// Eigenvector(s) of the pair (S, P) -- views: element (i, j) at sp[i * srs + j * scs] -- that belong to the diagonal block ending
// at row k (gevd/mod.rs:491-1005, column oriented as schur_core.h's eigvec_block): the null vector of M = a S - b P, where
// (b, a) is the eigenvalue (alpha, beta) scaled by ascale = 1 / |S|, bscale = 1 / |P| so that |a| |S| and |b| |P| are at most 1.
// A real eigenvalue writes column k of x; a pair in rows k - 1, k writes the real part to column cre and the imaginary part to
// column cim of (k - 1, k) for the eigenvalue whose imaginary part has the sign imsign.  (ar, ai, be)[i * es] belong to row i of
// the view.  Pivots below dmin = eps max(|a| |S|, |b| |P|) are replaced by it; a component above 1 / sqrt(min positive) rescales
// the vector.  Returns at once for the first row of a 2 x 2 block.
template <typename T, typename G>
SC_HD void gevec_block(const G &g, const T *sp, long srs, long scs, const T *pp, long prs, long pcs, long n, long k, const T *ar, const T *ai,
		       const T *be, long es, T imsign, bool swap, T *xp, long xrs, long xcs, T snorm, T pnorm)
{
#define SS(i, j) sp[(i) * srs + (j) * scs]
#define PP(i, j) pp[(i) * prs + (j) * pcs]
#define XX(i, j) xp[(i) * xrs + (j) * xcs]
#define MM(row_, col_) (cx_sub(Cx<T>{acoef * SS(row_, col_), 0}, Cx<T>{bc.r * PP(row_, col_), bc.i * PP(row_, col_)}))
	const int nt = g.size(), t = g.tid();
	const T safmin = Lim<T>::tiny(), ulp = Lim<T>::eps();
	if (k + 1 < n && SS(k + 1, k) != 0)
		return;
	const bool pair = k > 0 && SS(k, k - 1) != 0;
	const long top = pair ? k - 1 : k; // first row of the block
	const long cre = pair ? (swap ? k : k - 1) : k, cim = pair ? (swap ? k - 1 : k) : -1;
	const T ascale = 1 / sc_max(snorm, safmin), bscale = 1 / sc_max(pnorm, safmin);
	const T alr = ar[top * es], ali = pair ? sc_abs(ai[top * es]) * imsign : (T) 0, bet = be[top * es];
	const T temp = 1 / sc_max(sc_max((sc_abs(alr) + sc_abs(ali)) * ascale, sc_abs(bet) * bscale), safmin);
	// (beta by bscale and alpha by ascale first, as the reference: each is of order one then; beta ascale alone can underflow)
	const T acoef = ((temp * bet) * bscale) * ascale;
	const Cx<T> bc{((temp * alr) * ascale) * bscale, ((temp * ali) * ascale) * bscale};
	const T dmin = sc_max(sc_max(ulp * sc_abs(acoef) * snorm, ulp * cx_abs1(bc) * pnorm), safmin);
	const T big = 1 / sc_sqrt(safmin);
	Cx<T> xa{1, 0}, xb{1, 0}; // components top, k of the block
	if (pair) {
		const Cx<T> m00 = MM(k - 1, k - 1), m01 = MM(k - 1, k), m10 = MM(k, k - 1), m11 = MM(k, k);
		if (cx_abs1(m10) >= cx_abs1(m01)) {
			xb = Cx<T>{1, 0};
			xa = cx_div(Cx<T>{-m11.r, -m11.i}, m10);
		} else {
			xa = Cx<T>{1, 0};
			xb = cx_div(Cx<T>{-m00.r, -m00.i}, m01);
		}
	}
	for (long i = t; i < n; i += nt) {
		Cx<T> v{0, 0};
		if (i < top) {
			const Cx<T> u = cx_mul(MM(i, k), xb);
			v = Cx<T>{-u.r, -u.i};
			if (pair) {
				const Cx<T> w = cx_mul(MM(i, k - 1), xa);
				v.r -= w.r;
				v.i -= w.i;
			}
		} else if (i == top)
			v = pair ? xa : Cx<T>{1, 0};
		else if (i == k)
			v = xb;
		XX(i, cre) = v.r;
		if (pair)
			XX(i, cim) = v.i;
	}
	g.sync();
	long i = top;
	while (i > 0) {
		--i;
		const bool two = i > 0 && SS(i, i - 1) != 0;
		const long i0 = two ? i - 1 : i;
		Cx<T> y0{0, 0}, y1{0, 0};
		if (!two) {
			Cx<T> d = MM(i, i);
			if (cx_abs1(d) < dmin)
				d = Cx<T>{dmin, 0};
			const Cx<T> rhs{ldc(&XX(i, cre)), pair ? ldc(&XX(i, cim)) : (T) 0};
			y0 = cx_abs1(rhs) != 0 ? cx_div(rhs, d) : rhs;
		} else {
			Cx<T> m00 = MM(i0, i0), m01 = MM(i0, i), m10 = MM(i, i0), m11 = MM(i, i);
			Cx<T> r0{ldc(&XX(i0, cre)), pair ? ldc(&XX(i0, cim)) : (T) 0}, r1{ldc(&XX(i, cre)), pair ? ldc(&XX(i, cim)) : (T) 0};
			if (cx_abs1(m10) > cx_abs1(m00)) {
				Cx<T> w = m00;
				m00 = m10;
				m10 = w;
				w = m01;
				m01 = m11;
				m11 = w;
				w = r0;
				r0 = r1;
				r1 = w;
			}
			if (cx_abs1(m00) < dmin)
				m00 = Cx<T>{dmin, 0};
			const Cx<T> lf = cx_div(m10, m00);
			Cx<T> u11 = cx_sub(m11, cx_mul(lf, m01));
			if (cx_abs1(u11) < dmin)
				u11 = Cx<T>{dmin, 0};
			y1 = cx_div(cx_sub(r1, cx_mul(lf, r0)), u11);
			y0 = cx_div(cx_sub(r0, cx_mul(m01, y1)), m00);
		}
		const T mag = sc_max(cx_abs1(y0), cx_abs1(y1));
		T sc = 1;
		if (mag > big) {
			sc = 1 / mag;
			for (long r = i + 1 + t; r <= k; r += nt) {
				XX(r, cre) = ldc(&XX(r, cre)) * sc;
				if (pair)
					XX(r, cim) = ldc(&XX(r, cim)) * sc;
			}
			y0.r *= sc;
			y0.i *= sc;
			y1.r *= sc;
			y1.i *= sc;
		}
		for (long r = t; r < i0; r += nt) {
			Cx<T> u = cx_mul(MM(r, i0), y0);
			if (two) {
				const Cx<T> w = cx_mul(MM(r, i), y1);
				u.r += w.r;
				u.i += w.i;
			}
			XX(r, cre) = XX(r, cre) * sc - u.r;
			if (pair)
				XX(r, cim) = XX(r, cim) * sc - u.i;
		}
		g.sync(); // every thread has read the right-hand side that is overwritten now
		if (t == 0) {
			XX(i0, cre) = y0.r;
			if (pair)
				XX(i0, cim) = y0.i;
			if (two) {
				XX(i, cre) = y1.r;
				if (pair)
					XX(i, cim) = y1.i;
			}
		}
		g.sync();
		i = i0;
	}
#undef SS
#undef PP
#undef XX
#undef MM
}

struct GevdCounts {
	long sweeps = 0, window_steps = 0, leaves = 0, readbacks = 0;
};

// The sweep loop (the counterpart of schur_core.h's schur_drive), on a backend that launches the kernels (qz.hip) or calls the
// bodies above (tests/host/qz_host.cpp):
//   be.scan(hi, ilo, ihi, done)           qz_unblocked in scan mode from row hi - 1: both deflation tests, the deflation of 1 x 1 and
//                                         2 x 2 blocks with their (alpha, beta), then the lowest block of three rows or more,
//                                         [ilo, ihi); the read-back of the state record is the one host synchronisation per
//                                         sweep; false: a leaf or the scan reached its iteration cap;
//   be.leaf(ilo, m)                       qz_unblocked to convergence on the diagonal block + its off-block updates;
//   be.shifts(ilo, ihi, ns, exceptional)  the ns shifts of the next sweep;
//   be.window(w0, ws, ilo, ihi, nb, A, B) one window step + its off-window updates.
// Returns 0, or 1 when the cap of 30 max(10, n) rounds is reached.
template <typename B> int qz_drive(B &be, long n, long W, size_t (*shift_count)(size_t, size_t), GevdCounts &cnt)
{
	const long itmax = 30 * (n > 10 ? n : 10);
	long hi = n, kdefl = 0, pilo = -1, pihi = -1;
	for (long iter = 0;; ++iter) {
		if (iter == itmax)
			return 1;
		long ilo, ihi;
		bool done;
		const bool ok = be.scan(hi, ilo, ihi, done);
		++cnt.readbacks;
		if (!ok)
			return 1;
		if (done)
			return 0;
		if (ilo != pilo || ihi != pihi)
			kdefl = 0;
		pilo = ilo;
		pihi = ihi;
		const long m = ihi - ilo;
		if (m <= W) {
			be.leaf(ilo, m);
			++cnt.leaves;
			hi = ilo;
			pilo = pihi = -1;
			continue;
		}
		hi = ihi;
		++kdefl;
		long ns = (long) shift_count((size_t) n, (size_t) m);
		if (ns > 2 * max_bulges(W) || ns < 0)
			ns = 2 * max_bulges(W);
		if (ns > m - 1)
			ns = m - 1;
		ns = ns / 2 * 2;
		if (ns < 2)
			ns = 2;
		be.shifts(ilo, ihi, (int) ns, kdefl % 6 == 0);
		const int nb = (int) (ns / 2);
		const SweepPlan plan(W, ilo, ihi, nb);
		for (long t = 0; t < plan.steps; ++t) {
			long A, Bq, w0, ws;
			plan.window(t, ilo, ihi, nb, A, Bq, w0, ws);
			be.window(w0, ws, ilo, ihi, nb, A, Bq);
		}
		++cnt.sweeps;
		cnt.window_steps += plan.steps;
	}
}

} // namespace qz
} // namespace fh
