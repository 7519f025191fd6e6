// The step bodies of csrc/clu_core.h on the host: factors one complex matrix with clu_factor_unblocked and writes the pivots and the
// packed factors (tests/test_clu_host.py).  No GPU, no HIP header.
//   clu_host c32|c64 IN OUT
// IN : doubles {m, n, then the m x n matrix column major, (re, im) interleaved}; a missing IN ("-") reads the same from stdin.
// OUT: doubles {piv[0 .. min(m, n)), then the packed LU in the layout of the input}.
// The values pass through double unchanged (every float is a double), so c32 results come back bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "clu_core.h"

template <typename R> static int run(int m, int n, const std::vector<double> &in, std::vector<double> &out)
{
	const size_t mn = (size_t) m * (size_t) n;
	std::vector<R> re(mn), im(mn);
	for (size_t e = 0; e < mn; ++e) {
		re[e] = (R) in[2 * e];
		im[e] = (R) in[2 * e + 1];
	}
	const int k = m < n ? m : n;
	std::vector<int> piv((size_t) k);
	fh::clu::clu_factor_unblocked<R>(m, n, re.data(), im.data(), piv.data());
	out.clear();
	for (int j = 0; j < k; ++j)
		out.push_back((double) piv[(size_t) j]);
	for (size_t e = 0; e < mn; ++e) {
		out.push_back((double) re[e]);
		out.push_back((double) im[e]);
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 4 || (strcmp(argv[1], "c32") != 0 && strcmp(argv[1], "c64") != 0)) {
		fprintf(stderr, "usage: clu_host c32|c64 IN OUT\n");
		return 2;
	}
	FILE *fi = strcmp(argv[2], "-") == 0 ? stdin : fopen(argv[2], "rb");
	if (!fi) {
		perror(argv[2]);
		return 2;
	}
	double hdr[2];
	if (fread(hdr, sizeof(double), 2, fi) != 2 || hdr[0] < 0 || hdr[1] < 0 || hdr[0] > 1e6 || hdr[1] > 1e6) {
		fprintf(stderr, "clu_host: bad header\n");
		return 2;
	}
	const int m = (int) hdr[0], n = (int) hdr[1];
	std::vector<double> in(2 * (size_t) m * (size_t) n), out;
	if (fread(in.data(), sizeof(double), in.size(), fi) != in.size()) {
		fprintf(stderr, "clu_host: short input\n");
		return 2;
	}
	if (fi != stdin)
		fclose(fi);
	if (strcmp(argv[1], "c32") == 0)
		run<float>(m, n, in, out);
	else
		run<double>(m, n, in, out);
	FILE *fo = fopen(argv[3], "wb");
	if (!fo) {
		perror(argv[3]);
		return 2;
	}
	const bool ok = fwrite(out.data(), sizeof(double), out.size(), fo) == out.size();
	return fclose(fo) == 0 && ok ? 0 : 2;
}
