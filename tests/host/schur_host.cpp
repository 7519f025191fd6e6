// Host program around the bodies of csrc/schur_core.h (tests/test_schur_host.py): the whole sweep loop of the general EVD
// on one thread, with the window edge as a parameter so that a small matrix takes sweeps, windows and leaves.
//
//   schur_host f64|f32 W in.bin out.bin
//
// in.bin: doubles, n then the n x n upper Hessenberg matrix, column major.  out.bin: doubles, status (0, or 1 for the iteration
// cap), sweeps, window steps, leaves, then wr[n], wi[n], T[n * n], Z[n * n], X[n * n] (right eigenvectors of T), column major.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "schur_core.h"

using namespace fh::schur;

static size_t shift_count(size_t, size_t nh) { return nh < 30 ? 2 : (nh < 60 ? 4 : 10); }

// what schur.hip's DeviceSchur does with kernels and gemm_dev, with loops
template <typename T> struct HostSchur {
	long n, W;
	std::vector<T> h, z, wr, wi, sr, si, a, u, tmp;
	int st[ST_COUNT];
	HostGroup g;

	HostSchur(long n_, long W_) : n(n_), W(W_), h(n_ * n_), z(n_ * n_), wr(n_), wi(n_), sr(W_), si(W_), a(W_ * W_), u(W_ * W_), tmp(n_ * W_)
	{
		memset(st, 0, sizeof(st));
		for (long i = 0; i < n; ++i)
			z[i + i * n] = 1;
	}
	bool prepare(long hi, long &ilo, long &ihi, bool &done, long &deflated)
	{
		int red[3];
		sweep_prepare(g, h.data(), n, n, hi, st, red);
		ilo = st[ST_ILO];
		ihi = st[ST_IHI];
		done = st[ST_DONE] != 0;
		deflated = st[ST_DEFLATED];
		return st[ST_STATUS] == 0;
	}
	void load(long w0, long ws, bool hessenberg)
	{
		for (long j = 0; j < ws; ++j)
			for (long i = 0; i < ws; ++i) {
				a[i + j * ws] = hessenberg && i > j + 1 ? (T) 0 : h[(w0 + i) + (w0 + j) * n];
				u[i + j * ws] = i == j ? (T) 1 : (T) 0;
			}
	}
	void store(long w0, long ws)
	{
		for (long j = 0; j < ws; ++j)
			for (long i = 0; i < ws; ++i)
				h[(w0 + i) + (w0 + j) * n] = a[i + j * ws];
	}
	// rows [r0, r0 + nr) of the columns [w0, w0 + ws) of m <- the same times u
	void times_u(std::vector<T> &m, long r0, long nr, long w0, long ws)
	{
		for (long j = 0; j < ws; ++j)
			for (long i = 0; i < nr; ++i) {
				T s = 0;
				for (long k = 0; k < ws; ++k)
					s += m[(r0 + i) + (w0 + k) * n] * u[k + j * ws];
				tmp[i + j * nr] = s;
			}
		for (long j = 0; j < ws; ++j)
			for (long i = 0; i < nr; ++i)
				m[(r0 + i) + (w0 + j) * n] = tmp[i + j * nr];
	}
	void off_block(long w0, long ws)
	{
		const long right = n - (w0 + ws);
		for (long j = 0; j < right; ++j) { // H[win, right] <- u^T H[win, right]
			T *c = &h[w0 + (w0 + ws + j) * n];
			for (long i = 0; i < ws; ++i) {
				T s = 0;
				for (long k = 0; k < ws; ++k)
					s += u[k + i * ws] * c[k];
				tmp[i] = s;
			}
			for (long i = 0; i < ws; ++i)
				c[i] = tmp[i];
		}
		times_u(h, 0, w0, w0, ws);
		times_u(z, 0, n, w0, ws);
	}
	bool leaf(long ilo, long m)
	{
		load(ilo, m, true);
		if (lahqr(g, true, a.data(), m, m, u.data(), m, &wr[ilo], &wi[ilo]) != 0)
			return false;
		store(ilo, m);
		off_block(ilo, m);
		return true;
	}
	void shifts(long, long ihi, int ns, bool exceptional)
	{
		long err = exceptional;
		if (!exceptional) {
			load(ihi - ns, ns, true);
			err = lahqr(g, false, a.data(), (long) ns, (long) ns, (T *) nullptr, 0L, sr.data(), si.data());
		}
		if (err != 0)
			exceptional_shifts(h.data(), n, ihi, ns, sr.data(), si.data());
		pair_shifts(sr.data(), si.data(), ns, h[(ihi - 1) + (ihi - 1) * n]);
	}
	void window(long w0, long ws, long ilo, long ihi, int nb, long A, long B)
	{
		if (ws > W) {
			fprintf(stderr, "window of %ld rows in an edge of %ld\n", ws, W);
			exit(3);
		}
		load(w0, ws, false);
		window_chase(g, a.data(), ws, u.data(), ws, ws, w0, ilo, ihi, nb, sr.data(), si.data(), A, B);
		store(w0, ws);
		off_block(w0, ws);
	}
	void finish() { schur_finish(g, h.data(), n, n, z.data(), n, wr.data(), wi.data()); }
};

template <typename T> int run(long W, const std::vector<double> &in, const char *out)
{
	const long n = (long) in[0];
	HostSchur<T> be(n, W);
	for (long e = 0; e < n * n; ++e)
		be.h[e] = (T) in[1 + e];
	SchurCounts cnt;
	const int status = schur_drive(be, n, W, shift_count, cnt);
	std::vector<T> x(n * n, (T) 0);
	if (status == 0) {
		T norm = 0;
		for (long j = 0; j < n; ++j)
			for (long i = 0; i < (j + 2 < n ? j + 2 : n); ++i)
				norm += sc_abs(be.h[i + j * n]);
		for (long k = 0; k < n; ++k)
			eigvec_block(be.g, (const T *) be.h.data(), 1L, n, n, k, x.data(), 1L, n, norm);
	}
	std::vector<double> o;
	o.push_back(status);
	o.push_back((double) cnt.sweeps);
	o.push_back((double) cnt.window_steps);
	o.push_back((double) cnt.leaves);
	for (const std::vector<T> *v : {&be.wr, &be.wi, &be.h, &be.z, &x})
		for (T e : *v)
			o.push_back((double) e);
	FILE *f = fopen(out, "wb");
	if (!f || fwrite(o.data(), sizeof(double), o.size(), f) != o.size())
		return 2;
	fclose(f);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 5)
		return 2;
	FILE *f = fopen(argv[3], "rb");
	if (!f)
		return 2;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<double> in(bytes / sizeof(double));
	if (fread(in.data(), sizeof(double), in.size(), f) != in.size())
		return 2;
	fclose(f);
	const long W = atol(argv[2]);
	return strcmp(argv[1], "f32") == 0 ? run<float>(W, in, argv[4]) : run<double>(W, in, argv[4]);
}
