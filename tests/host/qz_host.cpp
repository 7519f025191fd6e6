// The bodies of csrc/qz_core.h on the host: Hessenberg-triangular reduction, QZ iteration and eigenvectors of a pair (A, B) with
// B upper triangular, on one thread (HostGroup).  tests/test_qz_host.py builds and runs this program.
//
//   qz_host <f64|f32> <edge> <cap> <in> <out>
// in:  doubles: n, then A and B column major.  edge: the window edge W of the sweep driver (qz_drive): blocks of at most W rows
//      go to the leaf, larger ones take multishift sweeps in windows of edge W.  cap: iteration cap of a scan or a leaf
//      (0: 30 max(10, n)).  QZ_HOST_NS in the environment: the shift count the driver is given (default 4).
// out: doubles: status, sweeps, infinite deflations, leaves, window steps; alpha_re, alpha_im, beta (n each); UR, UL, S, P, Q, Z (n x n each).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qz_core.h"

using namespace fh::qz;

static size_t g_ns = 4;
static size_t host_shift_count(size_t, size_t) { return g_ns; }

// the host backend of qz_drive: the same calls as the device backend of csrc/qz.hip, on plain arrays
template <typename T> struct HostQz {
	long n, W, cap;
	Pencil<T> p; // the whole pair and its factors
	T *ar, *ai, *be, anorm, bnorm;
	int cnt[QC_COUNT] = {0};
	bool failed = false;
	std::vector<T> lh, lt, u, v, sr, si;
	fh::schur::HostGroup g;

	bool scan(long hi, long &ilo, long &ihi, bool &done)
	{
		long bf = 0, bl = 0;
		const long r = qz_unblocked(g, p, ar, ai, be, anorm, bnorm, cap, cnt, hi - 1, 3L, bf, bl);
		done = r == 0;
		ilo = bf;
		ihi = bl + 1;
		return r <= 0 && !failed;
	}
	// the m x m diagonal block at w0 -> dense local copies, identities in u, v
	Pencil<T> local(long w0, long m)
	{
		lh.assign((size_t) (m * m), 0);
		lt.assign((size_t) (m * m), 0);
		u.assign((size_t) (m * m), 0);
		v.assign((size_t) (m * m), 0);
		for (long j = 0; j < m; ++j)
			for (long i = 0; i < m; ++i) {
				lh[i + j * m] = *p.H(w0 + i, w0 + j);
				lt[i + j * m] = *p.B(w0 + i, w0 + j);
				u[i + j * m] = v[i + j * m] = i == j;
			}
		return Pencil<T>{lh.data(), m, lt.data(), m, m, u.data(), m, v.data(), m};
	}
	// the block back, and the rest of the pair and of the factors under u (from the left, transposed) and v (from the right)
	void off_block(long w0, long m)
	{
		std::vector<T> x((size_t) m), y((size_t) m);
		for (long j = 0; j < m; ++j)
			for (long i = 0; i < m; ++i) {
				*p.H(w0 + i, w0 + j) = lh[i + j * m];
				*p.B(w0 + i, w0 + j) = lt[i + j * m];
			}
		for (int which = 0; which < 2; ++which) {
			T *a = which ? p.t : p.h;
			const long ld = which ? p.ldt : p.ldh;
			for (long c = w0 + m; c < n; ++c) { // rows of the window, right of it: u^T from the left
				for (long i = 0; i < m; ++i) {
					T sum = 0;
					for (long k = 0; k < m; ++k)
						sum += u[k + i * m] * a[(w0 + k) + c * ld];
					x[i] = sum;
				}
				for (long i = 0; i < m; ++i)
					a[(w0 + i) + c * ld] = x[i];
			}
			for (long r = 0; r < w0; ++r) { // columns of the window, above it: v from the right
				for (long jc = 0; jc < m; ++jc) {
					T sum = 0;
					for (long k = 0; k < m; ++k)
						sum += a[r + (w0 + k) * ld] * v[k + jc * m];
					y[jc] = sum;
				}
				for (long jc = 0; jc < m; ++jc)
					a[r + (w0 + jc) * ld] = y[jc];
			}
		}
		for (int which = 0; which < 2; ++which) {
			T *f = which ? p.z : p.q;
			const std::vector<T> &w = which ? v : u;
			for (long r = 0; r < n; ++r) {
				for (long jc = 0; jc < m; ++jc) {
					T sum = 0;
					for (long k = 0; k < m; ++k)
						sum += f[r + (w0 + k) * n] * w[k + jc * m];
					y[jc] = sum;
				}
				for (long jc = 0; jc < m; ++jc)
					f[r + (w0 + jc) * n] = y[jc];
			}
		}
	}
	void leaf(long ilo, long m)
	{
		Pencil<T> l = local(ilo, m);
		long bf, bl;
		if (qz_unblocked(g, l, ar + ilo, ai + ilo, be + ilo, anorm, bnorm, cap, cnt, m - 1, 0L, bf, bl) != 0)
			failed = true;
		off_block(ilo, m);
	}
	void shifts(long, long ihi, int ns, bool exceptional)
	{
		Pencil<T> l = local(ihi - ns, ns);
		l.q = l.z = nullptr;
		std::vector<T> a((size_t) ns), b((size_t) ns), c((size_t) ns);
		long bf, bl, err = 1;
		int scratch[QC_COUNT] = {0};
		if (!exceptional)
			err = qz_unblocked(g, l, a.data(), b.data(), c.data(), anorm, bnorm, cap, scratch, (long) ns - 1, 0L, bf, bl);
		sr.assign((size_t) ns, 0);
		si.assign((size_t) ns, 0);
		qz_sweep_shifts((const T *) p.h, p.ldh, (const T *) p.t, p.ldt, ihi, ns, exceptional, err, (const T *) a.data(), (const T *) b.data(),
				(const T *) c.data(), anorm, bnorm, sr.data(), si.data());
	}
	void window(long w0, long ws, long ilo, long ihi, int nb, long A, long B)
	{
		Pencil<T> l = local(w0, ws);
		qz_window_chase(g, l, w0, ilo, ihi, nb, (const T *) sr.data(), (const T *) si.data(), anorm, bnorm, A, B);
		off_block(w0, ws);
	}
};

template <typename T> static int run(long n, long edge, long cap, const std::vector<double> &in, const char *out_path)
{
	const size_t nn = (size_t) n * (size_t) n;
	std::vector<T> a(nn), b(nn), q(nn, 0), z(nn, 0), xr(nn), xl(nn), ar(n), ai(n), be(n);
	for (size_t i = 0; i < nn; ++i) {
		a[i] = (T) in[1 + i];
		b[i] = (T) in[1 + nn + i];
	}
	for (long i = 0; i < n; ++i)
		q[i + i * n] = z[i + i * n] = 1;
	fh::schur::HostGroup g;
	Pencil<T> p{a.data(), n, b.data(), n, n, q.data(), n, z.data(), n};
	hessenberg_triangular(g, p);
	// Frobenius norms, scaled by the largest entry so that the squares stay in range (as gevd_norms_kernel of csrc/qz.hip)
	double ma = 0, mb = 0, sa = 0, sb = 0;
	for (size_t i = 0; i < nn; ++i) {
		ma = std::fmax(ma, std::fabs((double) a[i]));
		mb = std::fmax(mb, std::fabs((double) b[i]));
	}
	for (size_t i = 0; i < nn; ++i) {
		sa += ma > 0 ? ((double) a[i] / ma) * ((double) a[i] / ma) : 0;
		sb += mb > 0 ? ((double) b[i] / mb) * ((double) b[i] / mb) : 0;
	}
	const T anorm = (T) (ma * std::sqrt(sa)), bnorm = (T) (mb * std::sqrt(sb));
	HostQz<T> hq;
	hq.n = n;
	hq.W = edge;
	hq.cap = cap > 0 ? cap : 30 * (n > 10 ? n : 10);
	hq.p = p;
	hq.ar = ar.data();
	hq.ai = ai.data();
	hq.be = be.data();
	hq.anorm = anorm;
	hq.bnorm = bnorm;
	GevdCounts gc;
	const long status = qz_drive(hq, n, edge, host_shift_count, gc);
	int *cnt = hq.cnt;
	if (status == 0)
		for (long k = 0; k < n; ++k) {
			gevec_block(g, (const T *) a.data(), 1L, n, (const T *) b.data(), 1L, n, n, k, (const T *) ar.data(), (const T *) ai.data(),
				    (const T *) be.data(), 1L, (T) 1, false, xr.data(), 1L, n, anorm, bnorm);
			// the left vectors: the same solve on the transposed pair with rows and columns reversed
			const long e = nn - 1;
			gevec_block(g, (const T *) a.data() + e, -n, -1L, (const T *) b.data() + e, -n, -1L, n, k, (const T *) ar.data() + (n - 1),
				    (const T *) ai.data() + (n - 1), (const T *) be.data() + (n - 1), -1L, (T) -1, true, xl.data() + e, -1L, -n, anorm, bnorm);
		}
	std::vector<double> out;
	out.push_back((double) status);
	out.push_back((double) gc.sweeps);
	out.push_back((double) cnt[QC_INFINITE]);
	out.push_back((double) gc.leaves);
	out.push_back((double) gc.window_steps);
	for (auto *v : {&ar, &ai, &be})
		for (long i = 0; i < n; ++i)
			out.push_back(status == 0 ? (double) (*v)[i] : 0.0);
	// UR = Z X, UL = Q Y
	for (int side = 0; side < 2; ++side) {
		const std::vector<T> &f = side == 0 ? z : q, &x = side == 0 ? xr : xl;
		for (long j = 0; j < n; ++j)
			for (long i = 0; i < n; ++i) {
				double s = 0;
				if (status == 0)
					for (long k = 0; k < n; ++k)
						s += (double) f[i + k * n] * (double) x[k + j * n];
				out.push_back((double) (T) s);
			}
	}
	for (auto *v : {&a, &b, &q, &z})
		for (size_t i = 0; i < nn; ++i)
			out.push_back((double) (*v)[i]);
	FILE *fo = fopen(out_path, "wb");
	if (!fo || fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
		return 2;
	fclose(fo);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 6) {
		fprintf(stderr, "usage: qz_host <f64|f32> <edge> <cap> <in> <out>\n");
		return 2;
	}
	FILE *fi = fopen(argv[4], "rb");
	if (!fi)
		return 2;
	std::vector<double> in;
	double v;
	while (fread(&v, sizeof(double), 1, fi) == 1)
		in.push_back(v);
	fclose(fi);
	if (in.empty())
		return 2;
	const long n = (long) in[0];
	if (n < 1 || in.size() != 1 + 2 * (size_t) n * (size_t) n)
		return 2;
	const long edge = atol(argv[2]), cap = atol(argv[3]);
	if (getenv("QZ_HOST_NS"))
		g_ns = (size_t) strtoull(getenv("QZ_HOST_NS"), nullptr, 10);
	return argv[1][1] == '6' ? run<double>(n, edge, cap, in, argv[5]) : run<float>(n, edge, cap, in, argv[5]);
}
