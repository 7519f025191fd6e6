// Stand-alone host program of tests/test_perm_host.py: perm_from_transpositions of csrc/perm.h, compiled without any HIP header.
//   perm_host n nstarts start_0 .. nrecords record_0 ..
// record j is relative to the last block start <= j (one start, 0: absolute records).  Prints perm, perm_inv and the count.
#define FH_PERM_HOST_ONLY
#include "../faer-rs_amd/csrc/perm.h"

#include <vector>

int main(int argc, char **argv)
{
	std::vector<long> a;
	for (int i = 1; i < argc; ++i)
		a.push_back(atol(argv[i]));
	if (a.size() < 3 || a.size() != (size_t) (3 + a[1] + a[2 + a[1]]))
		return 2;
	const long n = a[0], nstarts = a[1], nrecords = a[2 + nstarts];
	const long *starts = a.data() + 2, *rec = a.data() + 3 + nstarts;
	std::vector<fh::idx_t> perm((size_t) n), inv((size_t) n);
	long b = 0;
	auto record = [&](fh::idx_t j) {
		while (b + 1 < nstarts && starts[b + 1] <= j)
			++b;
		return (fh::idx_t) (starts[b] + rec[j]);
	};
	const long count = fh::perm_from_transpositions("perm_host", n, nrecords, record, perm.data(), inv.data());
	for (long i = 0; i < n; ++i)
		printf("%ld ", perm[(size_t) i]);
	printf("\n");
	for (long i = 0; i < n; ++i)
		printf("%ld ", inv[(size_t) i]);
	printf("\n%ld\n", count);
	return 0;
}
