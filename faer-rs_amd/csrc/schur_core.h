// Bodies of the real Schur kernels (schur.hip), written once for the device and for a host compiler.
//
// Every body takes a "group" G: tid(), size(), sync().  On the device it is the workgroup (threadIdx.x, blockDim.x,
// __syncthreads); on the host it is one thread and sync() does nothing, so the same arithmetic runs in a plain C++ program
// (tests/host/schur_host.cpp, run by tests/test_schur_host.py).
// Scalar decisions (shifts, deflation tests, reflectors) are taken by every thread redundantly from the same memory, so control
// flow is uniform; a scalar store is done by thread 0 between two sync().  The vector work -- a 3-row / 3-column reflector
// across the row and column length -- is split over the threads.
//
// Restated from the reference: lahqr (evd/schur/real_schur.rs:2353-2656) with lahqr_eig22 (:6), lahqr_schur22 (:161, dlanv2),
// lahqr_shiftcolumn (:271) and make_householder_in_place (householder.rs:59-107).
#pragma once
#include <cfloat>
#include <cmath>

#ifdef __HIPCC__
#define SC_HD __host__ __device__ inline
#else
#define SC_HD inline
#endif

namespace fh {
namespace schur {

template <typename T> struct Lim;
template <> struct Lim<double> {
	SC_HD static double eps() { return DBL_EPSILON; }
	SC_HD static double tiny() { return DBL_MIN; }
};
template <> struct Lim<float> {
	SC_HD static float eps() { return FLT_EPSILON; }
	SC_HD static float tiny() { return FLT_MIN; }
};

template <typename T> SC_HD T sc_abs(T x) { return x < 0 ? -x : x; }
template <typename T> SC_HD T sc_max(T a, T b) { return a > b ? a : b; }
template <typename T> SC_HD T sc_min(T a, T b) { return a < b ? a : b; }
SC_HD double sc_sqrt(double x) { return sqrt(x); }
SC_HD float sc_sqrt(float x) { return sqrtf(x); }
SC_HD double sc_hypot(double a, double b) { return hypot(a, b); }
SC_HD float sc_hypot(float a, float b) { return hypotf(a, b); }

// the group of a host program: one thread
struct HostGroup {
	int tid() const { return 0; }
	int size() const { return 1; }
	void sync() const {}
	void atomic_max(int *p, int v) const { *p = *p > v ? *p : v; }
	void atomic_add(int *p, int v) const { *p += v; }
};

// real_schur.rs:6-32
template <typename T> SC_HD void eig22(T a00, T a01, T a10, T a11, T &s1r, T &s1i, T &s2r, T &s2i)
{
	const T s = sc_abs(a00) + sc_abs(a01) + sc_abs(a10) + sc_abs(a11);
	if (s == 0) {
		s1r = s1i = s2r = s2i = 0;
		return;
	}
	a00 /= s;
	a01 /= s;
	a10 /= s;
	a11 /= s;
	const T tr = (a00 + a11) * (T) 0.5;
	const T det = (a00 - tr) * (a00 - tr) + a01 * a10;
	if (det >= 0) {
		const T rt = sc_sqrt(det);
		s1r = s * (tr + rt);
		s2r = s * (tr - rt);
		s1i = s2i = 0;
	} else {
		const T rt = sc_sqrt(-det);
		s1r = s2r = s * tr;
		s1i = s * rt;
		s2i = -s1i;
	}
}

// real_schur.rs:161-270 (dlanv2): standardises [[a, b], [c, d]]; (cs, sn) is the rotation
template <typename T> SC_HD void schur22(T &a, T &b, T &c, T &d, T &s1r, T &s1i, T &s2r, T &s2i, T &cs, T &sn)
{
	const T eps = Lim<T>::eps();
	const T safmn2 = sc_sqrt(Lim<T>::tiny() / eps);
	const T safmx2 = 1 / safmn2;
	if (c == 0) {
		cs = 1;
		sn = 0;
	} else if (b == 0) {
		cs = 0;
		sn = 1;
		const T t = d;
		d = a;
		a = t;
		b = -c;
		c = 0;
	} else if (a == d && (b > 0) != (c > 0)) {
		cs = 1;
		sn = 0;
	} else {
		T temp = a - d;
		T p = temp * (T) 0.5;
		const T bcmax = sc_max(sc_abs(b), sc_abs(c));
		T bcmin = sc_min(sc_abs(b), sc_abs(c));
		if ((b > 0) != (c > 0))
			bcmin = -bcmin;
		T scale = sc_max(sc_abs(p), bcmax);
		T z = (p / scale) * p + (bcmax / scale) * bcmin;
		if (z >= 4 * eps) {
			T t = sc_sqrt(scale) * sc_sqrt(z);
			if (p < 0)
				t = -t;
			z = p + t;
			a = d + z;
			d -= (bcmax / z) * bcmin;
			const T tau = sc_hypot(c, z); // (the reference squares and adds; hypot keeps the ends of the range)
			cs = z / tau;
			sn = c / tau;
			b = b - c;
			c = 0;
		} else {
			T sigma = b + c;
			for (int it = 0; it < 20; ++it) {
				scale = sc_max(sc_abs(temp), sc_abs(sigma));
				if (scale >= safmx2) {
					sigma *= safmn2;
					temp *= safmn2;
					continue;
				}
				if (scale <= safmn2) {
					sigma *= safmx2;
					temp *= safmx2;
					continue;
				}
				break;
			}
			p = temp * (T) 0.5;
			T tau = sc_hypot(sigma, temp);
			cs = sc_sqrt((1 + sc_abs(sigma) / tau) * (T) 0.5);
			sn = -p / (tau * cs);
			if (sigma < 0)
				sn = -sn;
			const T aa = a * cs + b * sn, bb = -a * sn + b * cs;
			const T cc = c * cs + d * sn, dd = -c * sn + d * cs;
			a = aa * cs + cc * sn;
			b = bb * cs + dd * sn;
			c = -aa * sn + cc * cs;
			d = -bb * sn + dd * cs;
			temp = (a + d) * (T) 0.5;
			a = temp;
			d = temp;
			if (c != 0 && b != 0 && (b > 0) == (c > 0)) {
				const T sab = sc_sqrt(sc_abs(b)), sac = sc_sqrt(sc_abs(c));
				p = c > 0 ? sab * sac : -sab * sac;
				tau = 1 / sc_sqrt(sc_abs(b + c));
				a = temp + p;
				d = temp - p;
				b -= c;
				c = 0;
				const T cs1 = sab * tau, sn1 = sac * tau;
				temp = cs * cs1 - sn * sn1;
				sn = cs * sn1 + sn * cs1;
				cs = temp;
			}
		}
	}
	if (c != 0) {
		const T t = sc_sqrt(sc_abs(b)) * sc_sqrt(sc_abs(c));
		s1r = a;
		s1i = t;
		s2r = d;
		s2i = -t;
	} else {
		s1r = a;
		s2r = d;
		s1i = s2i = 0;
	}
}

// real_schur.rs:271-319: first column of (H - s1)(H - s2) for the leading nr x nr block at h
template <typename T> struct Vec3 {
	T a, b, c;
};
template <typename T> SC_HD void shiftcolumn(const T *h, long ld, int nr, T s1r, T s1i, T s2r, T s2i, Vec3<T> &v)
{
	const T h00 = h[0], h10 = h[1], h01 = h[ld], h11 = h[ld + 1];
	if (nr == 2) {
		const T s = sc_abs(h00 - s2r) + sc_abs(s2i) + sc_abs(h10);
		if (s == 0) {
			v.a = v.b = 0;
		} else {
			const T h10s = h10 / s;
			v.a = h10s * h01 + (h00 - s1r) * ((h00 - s2r) / s) - s1i * (s2i / s);
			v.b = h10s * (h00 + h11 - s1r - s2r);
		}
		v.c = 0;
	} else {
		const T h20 = h[2], h21 = h[ld + 2], h02 = h[2 * ld], h12 = h[2 * ld + 1], h22 = h[2 * ld + 2];
		const T s = sc_abs(h00 - s2r) + sc_abs(s2i) + sc_abs(h10) + sc_abs(h20);
		if (s == 0) {
			v.a = v.b = v.c = 0;
		} else {
			const T h10s = h10 / s, h20s = h20 / s;
			v.a = (h00 - s1r) * ((h00 - s2r) / s) - s1i * (s2i / s) + h01 * h10s + h02 * h20s;
			v.b = h10s * (h00 + h11 - s1r - s2r) + h12 * h20s;
			v.c = h20s * (h00 + h22 - s1r - s2r) + h21 * h10s;
		}
	}
}

// householder.rs:59-107 on the first nr entries of v: v.a <- beta, v.b, v.c <- essentials; returns 1 / tau (0: the identity)
template <typename T> SC_HD T make_reflector(Vec3<T> &v, int nr)
{
	T tail = nr == 3 ? sc_hypot(v.b, v.c) : sc_abs(v.b);
	T head = v.a;
	T hn = sc_abs(head);
	if (hn < Lim<T>::tiny()) {
		head = 0;
		hn = 0;
		v.a = 0;
	}
	if (tail < Lim<T>::tiny())
		return 0;
	const T norm = sc_hypot(hn, tail);
	const T sign = hn != 0 ? head / hn : (T) 1;
	const T sn = sign * norm;
	const T inv = 1 / (head + sn);
	v.b *= inv;
	v.c *= inv;
	v.a = -sn;
	const T q = tail * sc_abs(inv);
	return 1 / ((T) 0.5 * (1 + q * q));
}

// the small-subdiagonal test of lahqr (real_schur.rs:2420-2449) on a(i, i - 1); lo / hi: the bounds `ilo`, `ihi` of that code
template <typename T> SC_HD bool small_subdiag(const T *a, long ld, long i, long lo, long hi)
{
	const T eps = Lim<T>::eps();
	const T small_num = Lim<T>::tiny() / eps;
	const T sub = sc_abs(a[i + (i - 1) * ld]);
	if (sub < small_num)
		return true;
	const T d0 = a[(i - 1) + (i - 1) * ld], d1 = a[i + i * ld];
	T tst = sc_abs(d0) + sc_abs(d1);
	if (tst == 0) {
		if (i >= lo + 2)
			tst += sc_abs(a[(i - 1) + (i - 2) * ld]);
		if (i + 1 < hi)
			tst += sc_abs(a[(i + 1) + i * ld]);
	}
	if (sub <= eps * tst) {
		const T up = sc_abs(a[(i - 1) + i * ld]);
		const T ab = sc_max(sub, up), ba = sc_min(sub, up);
		const T aa = sc_max(sc_abs(d1), sc_abs(d1 - d0)), bb = sc_min(sc_abs(d1), sc_abs(d1 - d0));
		const T s = aa + ab;
		if (ba * (ab / s) <= sc_max(eps * (bb * (aa / s)), small_num))
			return true;
	}
	return false;
}

// One reflector of a bulge chase (real_schur.rs:2565-2653) on rows / columns i .. i + nr - 1 of a.  intro: the reflector comes
// from the shifts (the first of a chain), else from column i - 1, which then receives (beta, 0, 0).  Applied from the left to
// columns [i, c1), from the right to rows [r0, r1), and to columns i .. of z (zr rows).  scale_prev: lahqr's a(i, i - 1) *= 1 - t1
// for a chain that starts below the top of its block.  The caller has synchronised before; on return the right-hand
// application may still be in flight (the next call, or the caller, synchronises first).
template <typename T, typename G>
SC_HD void bulge_step(const G &g, T *a, long ld, T *z, long ldz, long zr, long i, int nr, bool intro, bool scale_prev, T s1r, T s1i,
		      T s2r, T s2i, long c1, long r0, long r1)
{
	Vec3<T> v;
	if (intro) {
		shiftcolumn(a + i + i * ld, ld, nr, s1r, s1i, s2r, s2i, v);
	} else {
		v.a = a[i + (i - 1) * ld];
		v.b = a[i + 1 + (i - 1) * ld];
		v.c = nr == 3 ? a[i + 2 + (i - 1) * ld] : (T) 0;
	}
	const T t1 = make_reflector(v, nr);
	const T v2 = v.b, v3 = nr == 3 ? v.c : (T) 0;
	const T t2 = t1 * v2, t3 = t1 * v3;
	if (intro)
		g.sync(); // the 3 x 3 block read above is written below
	const int nt = g.size(), t = g.tid();
	// phase 1: rows of a (one column per thread), columns of z (one row per thread)
	const long ncol = c1 - i;
	for (long w = t; w < ncol + (z ? zr : 0); w += nt) {
		if (w < ncol) {
			T *c = a + i + (i + w) * ld;
			if (nr == 3) {
				const T sum = c[0] + v2 * c[1] + v3 * c[2];
				c[0] -= sum * t1;
				c[1] -= sum * t2;
				c[2] -= sum * t3;
			} else {
				const T sum = c[0] + v2 * c[1];
				c[0] -= sum * t1;
				c[1] -= sum * t2;
			}
		} else {
			T *r = z + (w - ncol) + i * ldz;
			if (nr == 3) {
				const T sum = r[0] + v2 * r[ldz] + v3 * r[2 * ldz];
				r[0] -= sum * t1;
				r[ldz] -= sum * t2;
				r[2 * ldz] -= sum * t3;
			} else {
				const T sum = r[0] + v2 * r[ldz];
				r[0] -= sum * t1;
				r[ldz] -= sum * t2;
			}
		}
	}
	g.sync();
	// phase 2: columns of a (one row per thread); thread 0 closes column i - 1
	for (long w = r0 + t; w < r1; w += nt) {
		T *r = a + w + i * ld;
		if (nr == 3) {
			const T sum = r[0] + v2 * r[ld] + v3 * r[2 * ld];
			r[0] -= sum * t1;
			r[ld] -= sum * t2;
			r[2 * ld] -= sum * t3;
		} else {
			const T sum = r[0] + v2 * r[ld];
			r[0] -= sum * t1;
			r[ld] -= sum * t2;
		}
	}
	if (t == 0) {
		if (!intro) {
			a[i + (i - 1) * ld] = v.a;
			a[i + 1 + (i - 1) * ld] = 0;
			if (nr == 3)
				a[i + 2 + (i - 1) * ld] = 0;
		} else if (scale_prev) {
			a[i + (i - 1) * ld] *= 1 - t1;
		}
	}
}

// lahqr on the n x n upper Hessenberg a (column major, ld), the whole matrix being the active block; z (n x n, ldz) <- z Q
// unless nullptr; want_t: keep a a Schur form (else only the eigenvalues are right).  Returns 0, or the reference's `istop`
// (> 0) when the iteration cap 30 max(10, n) is reached.
template <typename T, typename G> SC_HD long lahqr(const G &g, bool want_t, T *a, long ld, long n, T *z, long ldz, T *wr, T *wi)
{
	const T eps = Lim<T>::eps();
	const int t = g.tid();
	if (n == 0)
		return 0;
	if (n == 1) {
		if (t == 0) {
			wr[0] = a[0];
			wi[0] = 0;
		}
		return 0;
	}
	const long itmax = 30 * (n > 10 ? n : 10);
	long k_defl = 0, istop = n, istart = 0;
	for (long iter = 0;; ++iter) {
		if (iter == itmax)
			return istop;
		g.sync();
		if (istart + 1 >= istop) {
			if (istart + 1 == istop && t == 0) {
				wr[istart] = a[istart + istart * ld];
				wi[istart] = 0;
			}
			break;
		}
		const long istart_m = want_t ? 0 : istart, istop_m = want_t ? n : istop;
		long found = -1;
		for (long i = istop - 1; i > istart; --i)
			if (small_subdiag(a, ld, i, (long) 0, n)) {
				found = i;
				break;
			}
		if (found >= 0) {
			g.sync();
			if (t == 0)
				a[found + (found - 1) * ld] = 0;
			istart = found;
		}
		if (istart + 2 >= istop) {
			if (istart + 1 == istop) {
				if (t == 0) {
					wr[istart] = a[istart + istart * ld];
					wi[istart] = 0;
				}
			} else {
				T a00 = a[istart + istart * ld], a01 = a[istart + (istart + 1) * ld];
				T a10 = a[istart + 1 + istart * ld], a11 = a[istart + 1 + (istart + 1) * ld];
				T s1r, s1i, s2r, s2i, cs, sn;
				schur22(a00, a01, a10, a11, s1r, s1i, s2r, s2i, cs, sn);
				g.sync();
				if (t == 0) {
					a[istart + istart * ld] = a00;
					a[istart + (istart + 1) * ld] = a01;
					a[istart + 1 + istart * ld] = a10;
					a[istart + 1 + (istart + 1) * ld] = a11;
					wr[istart] = s1r;
					wi[istart] = s1i;
					wr[istart + 1] = s2r;
					wi[istart + 1] = s2i;
				}
				// rows istart, istart + 1 right of the block, the two columns above it, the two columns of z
				const long nrow = want_t ? istop_m - (istart + 2) : 0, ncol = want_t ? istart - istart_m : 0, nz = z ? n : 0;
				for (long w = t; w < nrow + ncol + nz; w += g.size()) {
					T *x, *y;
					if (w < nrow) {
						x = a + istart + (istart + 2 + w) * ld;
						y = x + 1;
					} else if (w < nrow + ncol) {
						x = a + istart_m + (w - nrow) + istart * ld;
						y = x + ld;
					} else {
						x = z + (w - nrow - ncol) + istart * ldz;
						y = x + ldz;
					}
					const T xv = *x, yv = *y;
					*x = cs * xv + sn * yv;
					*y = cs * yv - sn * xv;
				}
			}
			k_defl = 0;
			istop = istart;
			istart = 0;
			continue;
		}
		T a00, a01, a10, a11;
		++k_defl;
		if (k_defl % 10 == 0) {
			T s = sc_abs(a[istop - 1 + (istop - 2) * ld]);
			if (istop > 2)
				s += sc_abs(a[istop - 2 + (istop - 3) * ld]);
			a00 = (T) 0.75 * s + a[istop - 1 + (istop - 1) * ld];
			a01 = (T) -0.4375 * s;
			a10 = s;
			a11 = a00;
		} else {
			a00 = a[istop - 2 + (istop - 2) * ld];
			a10 = a[istop - 1 + (istop - 2) * ld];
			a01 = a[istop - 2 + (istop - 1) * ld];
			a11 = a[istop - 1 + (istop - 1) * ld];
		}
		T s1r, s1i, s2r, s2i;
		eig22(a00, a01, a10, a11, s1r, s1i, s2r, s2i);
		if (s1i == 0 && s2i == 0) {
			const T last = a[istop - 1 + (istop - 1) * ld];
			if (sc_abs(s1r - last) <= sc_abs(s2r - last))
				s2r = s1r;
			else
				s1r = s2r;
		}
		long istart2 = istart;
		if (istart + 3 < istop) {
			for (long i = istop - 3; i > istart; --i) {
				Vec3<T> v;
				shiftcolumn(a + i + i * ld, ld, 3, s1r, s1i, s2r, s2i, v);
				const T v0 = make_reflector(v, 3);
				const T refsum = v0 * a[i + (i - 1) * ld] + v.b * a[i + 1 + (i - 1) * ld];
				if (sc_abs(a[i + 1 + (i - 1) * ld] - refsum * v.b) + sc_abs(refsum * v.c)
				    <= eps * ((sc_abs(a[i + (i - 1) * ld]) + sc_abs(a[i + (i + 1) * ld])) + sc_abs(a[i + 1 + (i + 2) * ld]))) {
					istart2 = i;
					break;
				}
			}
		}
		for (long i = istart2; i < istop - 1; ++i) {
			const int nr = istop - i < 3 ? (int) (istop - i) : 3;
			g.sync();
			const long r1 = (i + 4 < istop ? i + 4 : istop);
			bulge_step(g, a, ld, z, ldz, n, i, nr, i == istart2, i > istart, s1r, s1i, s2r, s2i, istop_m, istart_m, r1);
		}
	}
	return 0;
}

// One window step of a multishift sweep on the ws x ws window a (LDS image of H[w0 .. w0 + ws, same columns]), u (ws x ws,
// identity on entry) <- the accumulated reflectors.  Bulge j of nb uses the shift pair (sr, si)[2 j], [2 j + 1] and takes the
// steps whose column index k (global) runs over [A - 3 j, B - 3 j), clipped to [ilo - 1, ihi - 2): k == ilo - 1 introduces the
// bulge at the top of the active block [ilo, ihi), k + 1 >= ihi - 2 lets it run off the bottom.  The leading bulge moves first.
template <typename T, typename G>
SC_HD void window_chase(const G &g, T *a, long ld, T *u, long ldu, long ws, long w0, long ilo, long ihi, int nb, const T *sr, const T *si,
			long A, long B)
{
	for (int j = 0; j < nb; ++j) {
		long ka = A - 3 * j, kb = B - 3 * j;
		if (ka < ilo - 1)
			ka = ilo - 1;
		if (kb > ihi - 2)
			kb = ihi - 2;
		const T s1r = sr[2 * j], s1i = si[2 * j], s2r = sr[2 * j + 1], s2i = si[2 * j + 1];
		for (long k = ka; k < kb; ++k) {
			const long i = k + 1 - w0; // local row of the reflector
			const long left = ihi - (k + 1);
			const int nr = left < 3 ? (int) left : 3;
			const long r1g = (k + 5 < ihi ? k + 5 : ihi) - w0;
			g.sync();
			bulge_step(g, a, ld, u, ldu, ws, i, nr, k == ilo - 1, false, s1r, s1i, s2r, s2i, ws, (long) 0, r1g);
		}
	}
	g.sync();
}

// A load that sees what another thread of the workgroup stored to global memory before the last sync()
template <typename T> SC_HD T ldc(const T *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
	if constexpr (sizeof(T) == 8) {
		const unsigned long long b = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return __builtin_bit_cast(T, b);
	} else {
		const unsigned b = __hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return __builtin_bit_cast(T, b);
	}
#else
	return *p;
#endif
}

// State record of the driver (ints): what the host reads back once per sweep
enum { ST_STATUS = 0, ST_ILO = 1, ST_IHI = 2, ST_DONE = 3, ST_DEFLATED = 4, ST_SHIFT_ERR = 5, ST_NONFINITE = 6, ST_COUNT = 16 };

// Between two sweeps, on the n x n Hessenberg h in global memory: the classical deflation test on every subdiagonal entry above
// row `hi` (decisions first, stores after: a test never sees a neighbour half updated), then the lowest diagonal block of
// three or more rows -> st[ST_ILO], st[ST_IHI] (exclusive); st[ST_DONE] = 1 if none is left.  red: three ints of LDS.
template <typename T, typename G> SC_HD void sweep_prepare(const G &g, T *h, long ld, long n, long hi, int *st, int *red)
{
	const int nt = g.size(), t = g.tid();
	int ndef = 0;
	for (long base = 1; base < hi; base += 64L * nt) {
		unsigned long long m = 0;
		for (int q = 0; q < 64; ++q) {
			const long k = base + (long) q * nt + t;
			if (k < hi && h[k + (k - 1) * ld] != 0 && small_subdiag(h, ld, k, (long) 0, n))
				m |= 1ull << q;
		}
		g.sync();
		for (int q = 0; q < 64; ++q)
			if ((m >> q) & 1) {
				const long k = base + (long) q * nt + t;
				h[k + (k - 1) * ld] = 0;
				++ndef;
			}
		g.sync();
	}
	if (t == 0)
		red[0] = red[1] = red[2] = 0;
	g.sync();
	if (ndef)
		g.atomic_add(&red[2], ndef);
	for (long k = 3 + t; k <= hi; k += nt) {
		const bool zb = k == n || ldc(h + k + (k - 1) * ld) == 0;
		if (zb && ldc(h + (k - 1) + (k - 2) * ld) != 0 && ldc(h + (k - 2) + (k - 3) * ld) != 0)
			g.atomic_max(&red[0], (int) k);
	}
	g.sync();
	const long istop = red[0];
	for (long k = 1 + t; k + 3 <= istop; k += nt)
		if (ldc(h + k + (k - 1) * ld) == 0)
			g.atomic_max(&red[1], (int) k);
	g.sync();
	if (t == 0) {
		st[ST_ILO] = red[1];
		st[ST_IHI] = (int) istop;
		st[ST_DONE] = istop == 0;
		st[ST_DEFLATED] = red[2];
	}
}

// The ns shifts of a sweep from the eigenvalues (wr, wi) of the trailing ns x ns block (real_schur.rs:2290-2335): sorted by
// decreasing |re| + |im|, then shuffled so that every pair (2 j, 2 j + 1) is two real shifts or a conjugate pair.  One thread.
template <typename T> SC_HD void pair_shifts(T *wr, T *wi, int ns, T last_diag)
{
	bool sorted = false;
	for (int k = ns; !sorted && k > 0; --k) {
		sorted = true;
		for (int i = 0; i + 1 < k; ++i)
			if (sc_abs(wr[i]) + sc_abs(wi[i]) < sc_abs(wr[i + 1]) + sc_abs(wi[i + 1])) {
				sorted = false;
				const T r = wr[i], m = wi[i];
				wr[i] = wr[i + 1];
				wi[i] = wi[i + 1];
				wr[i + 1] = r;
				wi[i + 1] = m;
			}
	}
	for (int i = ns - 1; i >= 2; i -= 2)
		if (wi[i] != -wi[i - 1]) {
			const T r = wr[i], m = wi[i];
			wr[i] = wr[i - 1];
			wi[i] = wi[i - 1];
			wr[i - 1] = wr[i - 2];
			wi[i - 1] = wi[i - 2];
			wr[i - 2] = r;
			wi[i - 2] = m;
		}
	if (ns == 2 && wi[0] == 0) {
		if (sc_abs(wr[0] - last_diag) < sc_abs(wr[1] - last_diag))
			wr[1] = wr[0];
		else
			wr[0] = wr[1];
	}
	// a pair that is neither (cannot be left by the shuffle of a set closed under conjugation; a failed leaf can): real parts only
	for (int i = 0; i + 1 < ns; i += 2)
		if (wi[i] != -wi[i + 1])
			wi[i] = wi[i + 1] = 0;
}

// Exceptional shifts of a sweep (real_schur.rs:2240-2260) for the block that ends at row istop (exclusive) of h.  One thread.
template <typename T> SC_HD void exceptional_shifts(const T *h, long ld, long istop, int ns, T *wr, T *wi)
{
	for (long i = istop - 1; i >= istop - ns + 1; i -= 2) {
		const long o = i - (istop - ns);
		if (i >= 2) {
			const T ss = sc_abs(h[i + (i - 1) * ld]) + sc_abs(h[(i - 1) + (i - 2) * ld]);
			const T aa = (T) 0.75 * ss + h[i + i * ld];
			eig22(aa, ss, (T) -0.4375 * ss, aa, wr[o - 1], wi[o - 1], wr[o], wi[o]);
		} else {
			wr[o] = wr[o - 1] = h[i + i * ld];
			wi[o] = wi[o - 1] = 0;
		}
	}
}

// After the last sweep every diagonal block of h has one or two rows.  Writes (wr, wi) and standardises the 2 x 2 blocks the
// sweeps isolated (the leaf has done its own), rotating rows and columns of h and the columns of z, block after block.
template <typename T, typename G> SC_HD void schur_finish(const G &g, T *h, long ld, long n, T *z, long ldz, T *wr, T *wi)
{
	const int nt = g.size(), t = g.tid();
	long k = 0;
	while (k < n) {
		if (k + 1 == n || h[(k + 1) + k * ld] == 0) { // (subdiagonal entries are not written here)
			if (t == 0) {
				wr[k] = ldc(h + k + k * ld);
				wi[k] = 0;
			}
			++k;
			continue;
		}
		T a00 = ldc(h + k + k * ld), a01 = ldc(h + k + (k + 1) * ld), a10 = h[(k + 1) + k * ld], a11 = ldc(h + (k + 1) + (k + 1) * ld);
		T s1r, s1i, s2r, s2i, cs, sn;
		schur22(a00, a01, a10, a11, s1r, s1i, s2r, s2i, cs, sn);
		if (t == 0) {
			wr[k] = s1r;
			wi[k] = s1i;
			wr[k + 1] = s2r;
			wi[k + 1] = s2i;
		}
		if (!(cs == 1 && sn == 0)) {
			g.sync();
			const long nrow = n - (k + 2), ncol = k, nz = z ? n : 0;
			for (long w = t; w < nrow + ncol + nz; w += nt) {
				T *x, *y;
				if (w < nrow) {
					x = h + k + (k + 2 + w) * ld;
					y = x + 1;
				} else if (w < nrow + ncol) {
					x = h + (w - nrow) + k * ld;
					y = x + ld;
				} else {
					x = z + (w - nrow - ncol) + k * ldz;
					y = x + ldz;
				}
				const T xv = ldc(x), yv = ldc(y);
				*x = cs * xv + sn * yv;
				*y = cs * yv - sn * xv;
			}
			if (t == 0) {
				h[k + k * ld] = a00;
				h[k + (k + 1) * ld] = a01;
				h[(k + 1) + (k + 1) * ld] = a11;
			}
			g.sync();
			if (t == 0)
				h[(k + 1) + k * ld] = a10; // after the sync: every thread has passed the test on this entry
		}
		k += 2;
	}
}

// Overflow guard of the back substitution (the reference has none and overflows where the vector grows past the range, a
// random triangular matrix of 127 rows in fp32): when a new component exceeds 1 / sqrt(min positive) the whole vector is
// divided by it.  Returns the factor (1: nothing to do) after applying it to rows (i, k] of the ncol columns at x; the
// caller applies it to the rows above with their update.
template <typename T, typename G> SC_HD T eigvec_guard(const G &g, T mag, T *x, long xrs, long xcs, int ncol, long i, long k)
{
	const T big = 1 / sc_sqrt(Lim<T>::tiny());
	if (!(mag > big))
		return 1;
	const T sc = 1 / mag;
	for (long r = i + 1 + g.tid(); r <= k; r += g.size())
		for (int c = 0; c < ncol; ++c)
			x[r * xrs + c * xcs] = ldc(&x[r * xrs + c * xcs]) * sc;
	return sc;
}

// Eigenvector(s) of the quasi upper triangular t (n x n view: element (i, j) at tp[i * trs + j * tcs]) that belong to the
// diagonal block ending at row k: one column for a 1 x 1 block, columns k - 1 (real part) and k (imaginary part) for a 2 x 2
// block; evd/mod.rs:573-620 with the two shifted solves :670-881, column oriented: once x(i) is final, the rows above take
// their update x(r) -= t(r, i) x(i), all threads at once.  x: view like t.  norm: sum of |t(i, j)| over the Hessenberg part.
// Every thread reads the right-hand side of row i (and i - 1) from x and divides it redundantly; thread 0 stores the result over
// it, so each row step is read, sync, store, sync -- as in lahqr and schur_finish.
// Returns at once for the first row of a 2 x 2 block (its workgroup has nothing to do).
template <typename T, typename G>
SC_HD void eigvec_block(const G &g, const T *tp, long trs, long tcs, long n, long k, T *xp, long xrs, long xcs, T norm)
{
#define TT(i, j) tp[(i) * trs + (j) * tcs]
#define XX(i, j) xp[(i) * xrs + (j) * xcs]
	const int nt = g.size(), t = g.tid();
	const T floor_ = Lim<T>::eps() * norm;
	if (k + 1 < n && TT(k + 1, k) != 0)
		return;
	if (k == 0 || TT(k, k - 1) == 0) {
		const T p = TT(k, k);
		for (long i = t; i < n; i += nt)
			XX(i, k) = i < k ? -TT(i, k) : (i == k ? (T) 1 : (T) 0);
		g.sync();
		long i = k;
		while (i > 0) {
			--i;
			if (i == 0 || TT(i, i - 1) == 0) {
				T xi = ldc(&XX(i, k));
				T zz = TT(i, i) - p;
				if (sc_abs(zz) < floor_)
					zz = floor_;
				if (xi != 0)
					xi /= zz;
				const T sc = eigvec_guard(g, sc_abs(xi), &XX(0, k), xrs, xcs, 1, i, k);
				xi *= sc;
				for (long r = t; r < i; r += nt)
					XX(r, k) = XX(r, k) * sc - TT(r, i) * xi;
				g.sync(); // every thread has read the pivot that is overwritten now
				if (t == 0)
					XX(i, k) = xi;
			} else {
				const T a = TT(i, i) - p, b = TT(i - 1, i), c = TT(i, i - 1);
				const T r0 = ldc(&XX(i - 1, k)), r1 = ldc(&XX(i, k));
				const T inv = 1 / (a * a - b * c);
				T x0 = (a * r0 - b * r1) * inv, x1 = (a * r1 - c * r0) * inv;
				const T sc = eigvec_guard(g, sc_max(sc_abs(x0), sc_abs(x1)), &XX(0, k), xrs, xcs, 1, i, k);
				x0 *= sc;
				x1 *= sc;
				for (long r = t; r + 1 < i; r += nt)
					XX(r, k) = XX(r, k) * sc - (TT(r, i - 1) * x0 + TT(r, i) * x1);
				g.sync();
				if (t == 0) {
					XX(i - 1, k) = x0;
					XX(i, k) = x1;
				}
				--i;
			}
			g.sync();
		}
		return;
	}
	// complex pair p +- i q in rows k - 1, k (mod.rs:594-618)
	const T p = TT(k, k);
	const T q = sc_sqrt(sc_abs(TT(k, k - 1))) * sc_sqrt(sc_abs(TT(k - 1, k)));
	T d0, d1; // x(k - 1, k - 1), x(k, k)
	if (sc_abs(TT(k - 1, k)) >= sc_abs(TT(k, k - 1))) {
		d0 = 1;
		d1 = q / TT(k - 1, k);
	} else {
		d0 = -q / TT(k, k - 1);
		d1 = 1;
	}
	for (long i = t; i < n; i += nt) {
		XX(i, k - 1) = i < k - 1 ? -d0 * TT(i, k - 1) : (i == k - 1 ? d0 : (T) 0);
		XX(i, k) = i < k - 1 ? -d1 * TT(i, k) : (i == k ? d1 : (T) 0);
	}
	g.sync();
	long i = k - 1;
	while (i > 0) {
		--i;
		if (i == 0 || TT(i, i - 1) == 0) {
			T zr = TT(i, i) - p, zi = -q;
			T zz = sc_hypot(zr, zi);
			if (zz < floor_) {
				zr = floor_;
				zi = 0;
				zz = zr;
			}
			const T wr_ = (zr / zz) / zz, wi_ = (-zi / zz) / zz;
			const T xr = ldc(&XX(i, k - 1)), xi = ldc(&XX(i, k));
			T yr = xr * wr_ - xi * wi_, yi = xr * wi_ + xi * wr_;
			const T sc = eigvec_guard(g, sc_max(sc_abs(yr), sc_abs(yi)), &XX(0, k - 1), xrs, xcs, 2, i, k);
			yr *= sc;
			yi *= sc;
			for (long r = t; r < i; r += nt) {
				const T tv = TT(r, i);
				XX(r, k - 1) = XX(r, k - 1) * sc - tv * yr;
				XX(r, k) = XX(r, k) * sc - tv * yi;
			}
			g.sync();
			if (t == 0) {
				XX(i, k - 1) = yr;
				XX(i, k) = yi;
			}
		} else {
			const T ar = TT(i, i) - p, ai = -q, b = TT(i - 1, i), c = TT(i, i - 1);
			const T r0r = ldc(&XX(i - 1, k - 1)), r0i = ldc(&XX(i - 1, k)), r1r = ldc(&XX(i, k - 1)), r1i = ldc(&XX(i, k));
			T zr = ar * ar - ai * ai - b * c, zi = 2 * (ar * ai);
			T zz = sc_hypot(zr, zi);
			if (zz < floor_) {
				zr = floor_;
				zi = 0;
				zz = zr;
			}
			const T wr_ = (zr / zz) / zz, wi_ = (-zi / zz) / zz;
			const T x0r = (ar * r0r - ai * r0i) - b * r1r, x0i = (ar * r0i + ai * r0r) - b * r1i;
			const T x1r = (ar * r1r - ai * r1i) - c * r0r, x1i = (ar * r1i + ai * r1r) - c * r0i;
			T y0r = x0r * wr_ - x0i * wi_, y0i = x0r * wi_ + x0i * wr_;
			T y1r = x1r * wr_ - x1i * wi_, y1i = x1r * wi_ + x1i * wr_;
			const T sc = eigvec_guard(g, sc_max(sc_max(sc_abs(y0r), sc_abs(y0i)), sc_max(sc_abs(y1r), sc_abs(y1i))), &XX(0, k - 1), xrs, xcs, 2, i, k);
			y0r *= sc;
			y0i *= sc;
			y1r *= sc;
			y1i *= sc;
			for (long r = t; r + 1 < i; r += nt) {
				const T t0 = TT(r, i - 1), t1 = TT(r, i);
				XX(r, k - 1) = XX(r, k - 1) * sc - (t0 * y0r + t1 * y1r);
				XX(r, k) = XX(r, k) * sc - (t0 * y0i + t1 * y1i);
			}
			g.sync();
			if (t == 0) {
				XX(i - 1, k - 1) = y0r;
				XX(i - 1, k) = y0i;
				XX(i, k - 1) = y1r;
				XX(i, k) = y1i;
			}
			--i;
		}
		g.sync();
	}
#undef TT
#undef XX
}

// Geometry of a sweep: nb bulges in windows of edge W advance s = W - 3 nb - 1 columns per
// window step.
struct SweepPlan {
	long s, steps;
	SweepPlan(long W, long ilo, long ihi, int nb)
	{
		s = W - 3 * nb - 1;
		const long span = (ihi - 2) - (ilo - 1) + 3 * (nb - 1);
		steps = span > 0 ? (span + s - 1) / s : 0;
	}
	void window(long t, long ilo, long ihi, int nb, long &A, long &B, long &w0, long &ws) const
	{
		A = ilo - 1 + t * s;
		B = A + s;
		w0 = A - 3 * (nb - 1);
		if (w0 < ilo)
			w0 = ilo;
		long we = B + 4;
		if (we > ihi)
			we = ihi;
		ws = we - w0;
	}
};

// Most bulges a chain in a window of edge W carries: the chain fills half the window and advances by the other half
SC_HD int max_bulges(long W) { return (int) (W / 6); }

struct SchurCounts {
	long sweeps = 0, window_steps = 0, leaves = 0, prepares = 0;
};

// The sweep loop, on a backend that launches the kernels (schur.hip) or calls the bodies above (a host program):
//   be.prepare(hi, ilo, ihi, done, deflated)  sweep_prepare and the read-back of the state record: the one host synchronisation
//                                             per sweep; false: a leaf since the last prepare reached its iteration cap;
//   be.leaf(ilo, m)                           lahqr on the diagonal block + its off-block updates; false: iteration cap, where
//                                             the backend knows at once (the device reports it through the next prepare);
//   be.shifts(ilo, ihi, ns, exceptional)      the ns shifts of the next sweep;
//   be.window(w0, ws, ilo, ihi, nb, A, B)     one window step + its off-window updates;
//   be.finish()                               schur_finish.
// Returns 0, or 1 when the cap of 30 max(10, n) rounds is reached (lahqr's, real_schur.rs:2393).
template <typename B> int schur_drive(B &be, long n, long W, size_t (*shift_count)(size_t, size_t), SchurCounts &cnt)
{
	const long itmax = 30 * (n > 10 ? n : 10);
	long hi = n, kdefl = 0, pilo = -1, pihi = -1;
	for (long iter = 0;; ++iter) {
		if (iter == itmax)
			return 1;
		long ilo, ihi;
		bool done;
		long deflated;
		const bool ok = be.prepare(hi, ilo, ihi, done, deflated);
		++cnt.prepares;
		if (!ok)
			return 1;
		if (done)
			break;
		if (deflated > 0 || ilo != pilo || ihi != pihi)
			kdefl = 0;
		pilo = ilo;
		pihi = ihi;
		const long m = ihi - ilo;
		if (m <= W) {
			if (!be.leaf(ilo, m))
				return 1;
			++cnt.leaves;
			hi = ilo;
			pilo = pihi = -1;
			continue;
		}
		hi = ihi;
		++kdefl;
		long ns = (long) shift_count((size_t) n, (size_t) m);
		if (ns > 2 * max_bulges(W))
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
	be.finish();
	return 0;
}

} // namespace schur
} // namespace fh
