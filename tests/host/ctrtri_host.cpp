// The leaf bodies of csrc/ctrtri_core.h on the host: inverts one complex lower-triangular matrix the way ctrtri.hip does -- the E x E
// diagonal blocks with ct_leaf_host (reciprocals, substitution on the sub-blocks, doubling), the levels above as plain products -- and
// writes the result (tests/test_ctrtri_host.py).  No GPU, no HIP header.
//   ctrtri_host c32|c64 IN OUT
// IN : doubles {n, unit (0 / 1), then the n x n matrix column major, (re, im) interleaved}.  Only the lower triangle is read (unit: the
//      strict one); the rest may hold NaNs.
// OUT: doubles, the n x n result in the layout of the input: the inverse's lower triangle (unit: strict), every other entry as it came in.
// The values pass through double unchanged (every float is a double), so c32 results come back bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctrtri_core.h"

using namespace fh::ctrtri;

template <typename R> static void run(int n, bool unit, const std::vector<double> &in, std::vector<double> &out)
{
	const size_t nn = (size_t) n * (size_t) n;
	std::vector<R> sre(nn), sim(nn), dre(nn), dim(nn);
	for (size_t e = 0; e < nn; ++e) {
		sre[e] = dre[e] = (R) in[2 * e];
		sim[e] = dim[e] = (R) in[2 * e + 1];
	}
	auto at = [n](int i, int j) { return (size_t) j * (size_t) n + (size_t) i; };
	// leaves
	std::vector<R> bre((size_t) E * E), bim((size_t) E * E), tr((size_t) E * E / 4), ti((size_t) E * E / 4);
	for (int r0 = 0; r0 < n; r0 += E) {
		const int nb = n - r0 < E ? n - r0 : E;
		for (int j = 0; j < E; ++j)
			for (int i = 0; i < E; ++i) {
				const bool read = i < nb && j < nb && (i > j || (i == j && !unit));
				bre[(size_t) j * E + i] = read ? sre[at(r0 + i, r0 + j)] : (R) (i == j ? 1 : 0);
				bim[(size_t) j * E + i] = read ? sim[at(r0 + i, r0 + j)] : (R) 0;
			}
		ct_leaf_host<R>(bre.data(), bim.data(), E, unit, tr.data(), ti.data());
		for (int j = 0; j < nb; ++j)
			for (int i = unit ? j + 1 : j; i < nb; ++i) {
				dre[at(r0 + i, r0 + j)] = bre[(size_t) j * E + i];
				dim[at(r0 + i, r0 + j)] = bim[(size_t) j * E + i];
			}
	}
	// levels: dst_bl = -dst_br * (src_bl * dst_tl), the diagonal of a unit dst taken as one
	auto w = [&](int i, int j, R &xr, R &xi) {
		if (unit && i == j) {
			xr = (R) 1;
			xi = (R) 0;
		} else {
			xr = dre[at(i, j)];
			xi = dim[at(i, j)];
		}
	};
	for (long h = E; h < n; h *= 2)
		for (long base = 0; base + h < n; base += 2 * h) {
			const int b = (int) base, hh = (int) h, h2 = (int) (n - base - h < h ? n - base - h : h);
			std::vector<R> pr((size_t) h2 * hh), pi((size_t) h2 * hh);
			for (int j = 0; j < hh; ++j)
				for (int i = 0; i < h2; ++i) {
					R sr = (R) 0, si = (R) 0;
					for (int k = j; k < hh; ++k) {
						R xr, xi;
						w(b + k, b + j, xr, xi);
						ct_mac(sr, si, sre[at(b + hh + i, b + k)], sim[at(b + hh + i, b + k)], xr, xi);
					}
					pr[(size_t) j * h2 + i] = sr;
					pi[(size_t) j * h2 + i] = si;
				}
			for (int j = 0; j < hh; ++j)
				for (int i = 0; i < h2; ++i) {
					R sr = (R) 0, si = (R) 0;
					for (int k = 0; k <= i; ++k) {
						R xr, xi;
						w(b + hh + i, b + hh + k, xr, xi);
						ct_mac(sr, si, xr, xi, pr[(size_t) j * h2 + k], pi[(size_t) j * h2 + k]);
					}
					dre[at(b + hh + i, b + j)] = -sr;
					dim[at(b + hh + i, b + j)] = -si;
				}
		}
	out.resize(2 * nn);
	for (size_t e = 0; e < nn; ++e) {
		out[2 * e] = (double) dre[e];
		out[2 * e + 1] = (double) dim[e];
	}
}

int main(int argc, char **argv)
{
	if (argc != 4 || (strcmp(argv[1], "c32") != 0 && strcmp(argv[1], "c64") != 0)) {
		fprintf(stderr, "usage: ctrtri_host c32|c64 IN OUT\n");
		return 2;
	}
	FILE *fi = fopen(argv[2], "rb");
	if (!fi) {
		perror(argv[2]);
		return 2;
	}
	double hdr[2];
	if (fread(hdr, sizeof(double), 2, fi) != 2 || hdr[0] < 0 || hdr[0] > 1e5 || (hdr[1] != 0 && hdr[1] != 1)) {
		fprintf(stderr, "ctrtri_host: bad header\n");
		return 2;
	}
	const int n = (int) hdr[0];
	std::vector<double> in(2 * (size_t) n * (size_t) n), out;
	if (fread(in.data(), sizeof(double), in.size(), fi) != in.size()) {
		fprintf(stderr, "ctrtri_host: short input\n");
		return 2;
	}
	fclose(fi);
	if (strcmp(argv[1], "c32") == 0)
		run<float>(n, hdr[1] != 0, in, out);
	else
		run<double>(n, hdr[1] != 0, in, out);
	FILE *fo = fopen(argv[3], "wb");
	if (!fo) {
		perror(argv[3]);
		return 2;
	}
	const bool ok = fwrite(out.data(), sizeof(double), out.size(), fo) == out.size();
	return fclose(fo) == 0 && ok ? 0 : 2;
}
