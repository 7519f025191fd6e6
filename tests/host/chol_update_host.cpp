// The bodies of csrc/chol_update_core.h on the host (tests/test_chol_update_host.py): the block loop of csrc/chol_update.hip with
// HostGroup (one thread that owns every row of a diagonal block) and a small block edge, so that matrices of a few rows cross
// block and chunk borders.  Stand-alone: it has its own main and can be built with -fsanitize=address,undefined.
//
//   chol_update_host f64|f32 llt|ldlt|delete in.bin out.bin
// in.bin  (doubles): n, r, the factor (n x n, column major), then W (n x r, column major) and alpha (r) -- or, for delete, the r
//         sorted indices.
// out.bin (doubles): status (-1, or the failing column), the factor (n x n, column major).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "chol_update_core.h"

using namespace fh::cholup;

constexpr int NB = 8, RC = 2;

// chol_update.hip: rank_update_launches with diag_kernel and tail_kernel; L is m x m with leading dimension ld
template <bool LDLT, typename T> long rank_update(T *L, long ld, long m, T *W, long r, T *alpha)
{
	int status = 0;
	std::vector<Coef<T>> tab((size_t) NB * RC);
	static DiagLocal<T, NB, RC> local;
	const HostGroup g{NB};
	for (long j0 = 0; j0 < m; j0 += NB) {
		const int nb = (int) (m - j0 < NB ? m - j0 : NB);
		for (long k0 = 0; k0 < r; k0 += RC) {
			const int rc = (int) (r - k0 < RC ? r - k0 : RC);
			const int limit = LDLT ? nb : diag_limit(status, (int) j0, nb);
			if (limit > 0) {
				// (poison: every entry the step reads it has written itself)
				memset(&local, 0xFF, sizeof(local));
				memset(tab.data(), 0xFF, tab.size() * sizeof(Coef<T>));
				const int done = diag_block<LDLT, NB, RC, T>(g, local, L + j0 + j0 * ld, 1, ld, W + j0 + k0 * m, 1, m, alpha + k0, nb, rc, limit, tab.data());
				if (done < limit)
					status = (int) j0 + done + 1;
			}
			if (status != 0)
				continue;
			for (long i = j0 + nb; i < m; ++i)
				tail_row<LDLT, RC, T>(L + i + j0 * ld, ld, W + i + k0 * m, m, nb, rc, tab.data());
		}
	}
	return status == 0 ? -1 : status - 1;
}

template <typename T> int run(const std::string &mode, const std::vector<double> &in, const char *out_path)
{
	const long n = (long) in[0], r = (long) in[1];
	std::vector<T> L((size_t) (n * n));
	for (long e = 0; e < n * n; ++e)
		L[(size_t) e] = (T) in[2 + (size_t) e];
	const double *rest = in.data() + 2 + n * n;
	long status = -1;
	if (mode == "delete") {
		// chol_update.hip: keep_kernel, delete_gather_kernel, delete_copy_kernel, delete_compact_kernel
		std::vector<long> idx((size_t) r);
		for (long k = 0; k < r; ++k)
			idx[(size_t) k] = (long) rest[k];
		const long first = idx[0], nkeep = n - r, m = n - first - r;
		std::vector<long> keep((size_t) nkeep);
		for (long q = 0; q < nkeep; ++q)
			keep[(size_t) q] = kept_index(q, idx.data(), r);
		std::vector<T> W((size_t) (m * r)), alpha((size_t) r), C(L);
		for (long k = 0; k < r; ++k) {
			alpha[(size_t) k] = L[(size_t) (idx[k] + idx[k] * n)];
			for (long t = 0; t < m; ++t) {
				const long i = keep[(size_t) (first + t)];
				W[(size_t) (t + k * m)] = i > idx[k] ? L[(size_t) (i + idx[k] * n)] : (T) 0;
			}
		}
		for (long q = 0; q < nkeep; ++q)
			for (long p = q > first ? q : first; p < nkeep; ++p)
				L[(size_t) (p + q * n)] = C[(size_t) (keep[(size_t) p] + keep[(size_t) q] * n)];
		if (m > 0)
			rank_update<true, T>(L.data() + first + first * n, n, m, W.data(), r, alpha.data());
	} else {
		std::vector<T> W((size_t) (n * r)), alpha((size_t) r);
		for (long e = 0; e < n * r; ++e)
			W[(size_t) e] = (T) rest[e];
		for (long k = 0; k < r; ++k)
			alpha[(size_t) k] = (T) rest[n * r + k];
		status = mode == "ldlt" ? rank_update<true, T>(L.data(), n, n, W.data(), r, alpha.data()) : rank_update<false, T>(L.data(), n, n, W.data(), r, alpha.data());
	}
	std::vector<double> out((size_t) (1 + n * n));
	out[0] = (double) status;
	for (long e = 0; e < n * n; ++e)
		out[1 + (size_t) e] = (double) L[(size_t) e];
	FILE *f = fopen(out_path, "wb");
	if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size())
		return 2;
	fclose(f);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc != 5) {
		fprintf(stderr, "usage: chol_update_host f64|f32 llt|ldlt|delete in.bin out.bin\n");
		return 2;
	}
	FILE *f = fopen(argv[3], "rb");
	if (!f)
		return 2;
	fseek(f, 0, SEEK_END);
	const long bytes = ftell(f);
	fseek(f, 0, SEEK_SET);
	std::vector<double> in((size_t) bytes / sizeof(double));
	if (fread(in.data(), sizeof(double), in.size(), f) != in.size())
		return 2;
	fclose(f);
	const std::string dt = argv[1], mode = argv[2];
	return dt == "f64" ? run<double>(mode, in, argv[4]) : run<float>(mode, in, argv[4]);
}
