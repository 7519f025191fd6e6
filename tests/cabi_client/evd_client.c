/* A C client of the general EVD entry points.  Built against faer-ffi's own faer.h (-DEVD_CLIENT_REF_HEADER: its type
 * names carry the FaerV0_24_ prefix) or against include/faer_hip.h; tests/test_cabi_client_evd.py does both.
 * `host-only`: parameter constructors and the scratch query (no device).  Without arguments: also the decomposition of a
 * 4 x 4 matrix held in host memory, eigenvalues 1, 2 and 3 +- 4i. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef EVD_CLIENT_REF_HEADER
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include "faer.h"
#define TY(x) FaerV0_24_##x
#define TAG_OK FaerV0_24_EvdStatus_Ok
#define VEC_YES FaerV0_24_ComputeEigenvectors_Yes
#define PAR_SEQ FaerV0_24_ParTag_Seq
#else
#include "faer_hip.h"
#define TY(x) Faer##x
#define TAG_OK FaerEvdStatus_Ok
#define VEC_YES FaerComputeEigenvectors_Yes
#define PAR_SEQ FaerParTag_Seq
#endif

#define CHECK(c)                                                                                                        \
	do {                                                                                                            \
		if (!(c)) {                                                                                             \
			fprintf(stderr, "evd_client: %s failed (line %d)\n", #c, __LINE__);                               \
			return 1;                                                                                       \
		}                                                                                                       \
	} while (0)

int main(int argc, char **argv)
{
	TY(EvdParams) p = libfaer_v0_23_EvdParams_f64();
	TY(Par) par;
	memset(&par, 0, sizeof(par));
	par.tag = PAR_SEQ;
	CHECK(p.schur.recommended_shift_count(100, 100) == 12 && p.schur.recommended_deflation_window(100, 100) == 10);
	CHECK(p.schur.blocking_threshold == 75 && p.evd_from_schur.recursion_threshold == 64);
	TY(Layout) l0 = libfaer_v0_23_evd_scratch_f64(0, VEC_YES, VEC_YES, par, p);
	TY(Layout) l4 = libfaer_v0_23_evd_scratch_f64(4, VEC_YES, VEC_YES, par, p);
	CHECK(l0.len_bytes == 0 && l4.len_bytes >= 3 * 16 * sizeof(double));
	if (argc > 1 && strcmp(argv[1], "host-only") == 0) {
		printf("evd_client host-only ok\n");
		return 0;
	}
	/* B = diag(1, 2) + [[3, 4], [-4, 3]], A = S B S^-1 with S unit lower bidiagonal (column major below) */
	enum { N = 4 };
	double b[N][N] = {{1, 0, 0, 0}, {0, 2, 0, 0}, {0, 0, 3, 4}, {0, 0, -4, 3}}, a[N * N], sb[N][N], ul[N * N], ur[N * N], s[N], si[N];
	for (int i = 0; i < N; ++i)
		for (int j = 0; j < N; ++j)
			sb[i][j] = b[i][j] + (i > 0 ? 0.5 * b[i - 1][j] : 0.0); /* S B */
	for (int i = 0; i < N; ++i) /* (S B) S^-1: S^-1 = sum_k (-0.5)^k on the k-th subdiagonal */
		for (int j = 0; j < N; ++j) {
			double acc = 0, f = 1;
			for (int k = j; k < N; ++k, f *= -0.5)
				acc += sb[i][k] * f;
			a[i + j * N] = acc;
		}
	TY(MatRef) A = {a, N, N, 1, N};
	TY(MatMut) UL = {ul, N, N, 1, N}, UR = {ur, N, N, 1, N};
	TY(VecMut) S = {s, N, 1}, SI = {si, N, 1};
	TY(MemAlloc) mem = {NULL, 0};
	TY(EvdStatus) st = libfaer_v0_23_evd_f64(A, UL, UR, S, SI, par, mem, p);
	CHECK(st.tag == TAG_OK);
	int seen[4] = {0, 0, 0, 0};
	for (int i = 0; i < N; ++i) {
		const double want_re[4] = {1, 2, 3, 3}, want_im[4] = {0, 0, 4, -4};
		for (int k = 0; k < 4; ++k)
			if (fabs(s[i] - want_re[k]) < 1e-12 && fabs(si[i] - want_im[k]) < 1e-12)
				seen[k]++;
	}
	CHECK(seen[0] == 1 && seen[1] == 1 && seen[2] == 1 && seen[3] == 1);
	/* A ur = s ur for the real eigenvalues */
	for (int i = 0; i < N; ++i) {
		if (si[i] != 0)
			continue;
		double res = 0, nrm = 0;
		for (int r = 0; r < N; ++r) {
			double acc = 0;
			for (int c = 0; c < N; ++c)
				acc += a[r + c * N] * ur[c + i * N];
			res += fabs(acc - s[i] * ur[r + i * N]);
			nrm += fabs(ur[r + i * N]);
		}
		CHECK(nrm > 0 && res < 1e-12 * nrm);
	}
	printf("evd_client ok: %g%+gi %g%+gi %g%+gi %g%+gi\n", s[0], si[0], s[1], si[1], s[2], si[2], s[3], si[3]);
	return 0;
}
