/* A C client of the generalized EVD written against the REFERENCE's own header, faer-ffi/faer.h (pass -I<reference>/faer-ffi;
 * tests/test_cabi_client_gevd.py does).  The struct layouts of the family are _Static_assert-ed against include/faer_hip.h, the
 * `libfaer_v0_23_*` prototypes are the reference's.  Without arguments it runs the host-only entry points (params, scratch
 * sizes); with `compute` it decomposes a small pair on the GPU and checks beta A x = alpha B x for every right eigenvector. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "faer.h" /* the reference's header */
#define FAER_HIP_NO_FFI_PROTOTYPES
#include "faer_hip.h" /* ours: types + faer_hip_* runtime functions */

#define SAME_SIZE(A, B) _Static_assert(sizeof(A) == sizeof(B) && _Alignof(A) == _Alignof(B), "size/alignment of " #A " != " #B)
#define SAME_FIELD(A, B, F) _Static_assert(offsetof(A, F) == offsetof(B, F) && sizeof(((A *) 0)->F) == sizeof(((B *) 0)->F), "field " #F " of " #A " / " #B)

SAME_SIZE(FaerV0_24_GeneralizedHessenbergParams, FaerGeneralizedHessenbergParams);
SAME_FIELD(FaerV0_24_GeneralizedHessenbergParams, FaerGeneralizedHessenbergParams, block_size);
SAME_FIELD(FaerV0_24_GeneralizedHessenbergParams, FaerGeneralizedHessenbergParams, blocking_threshold);
SAME_SIZE(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams);
SAME_FIELD(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams, relative_cost_estimate_of_shift_chase_to_matmul);
SAME_FIELD(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams, recommended_shift_count);
SAME_FIELD(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams, recommended_deflation_window);
SAME_FIELD(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams, blocking_threshold);
SAME_FIELD(FaerV0_24_GeneralizedSchurParams, FaerGeneralizedSchurParams, nibble_threshold);
SAME_SIZE(FaerV0_24_GevdFromSchurParams, FaerGevdFromSchurParams);
SAME_FIELD(FaerV0_24_GevdFromSchurParams, FaerGevdFromSchurParams, padding);
SAME_SIZE(FaerV0_24_GevdParams, FaerGevdParams);
SAME_FIELD(FaerV0_24_GevdParams, FaerGevdParams, hessenberg);
SAME_FIELD(FaerV0_24_GevdParams, FaerGevdParams, schur);
SAME_FIELD(FaerV0_24_GevdParams, FaerGevdParams, evd_from_schur);
SAME_SIZE(FaerV0_24_GevdStatus, FaerGevdStatus);
SAME_FIELD(FaerV0_24_GevdStatus, FaerGevdStatus, tag);
SAME_FIELD(FaerV0_24_GevdStatus, FaerGevdStatus, ok);
SAME_FIELD(FaerV0_24_GevdStatus, FaerGevdStatus, no_convergence);
_Static_assert((int) FaerV0_24_GevdStatus_Ok == (int) FaerGevdStatus_Ok && (int) FaerV0_24_GevdStatus_NoConvergence == (int) FaerGevdStatus_NoConvergence, "GevdStatus");

#define CHECK(c)                                                                 \
	do {                                                                     \
		if (!(c)) {                                                      \
			fprintf(stderr, "gevd_client: %s failed (line %d)\n", #c, __LINE__); \
			return 1;                                                \
		}                                                                \
	} while (0)

static int host_only(void)
{
	const FaerV0_24_GevdParams p = libfaer_v0_23_GevdParams_f64(), q = libfaer_v0_23_GevdParams_f32();
	CHECK(p.hessenberg.block_size == 32 && p.hessenberg.blocking_threshold == 256 * 256);
	CHECK(q.hessenberg.block_size == 32 && q.schur.relative_cost_estimate_of_shift_chase_to_matmul(100, 50) == 10);
	CHECK(p.schur.recommended_shift_count(100, 100) == libfaer_v0_23_SchurParams_f64().recommended_shift_count(100, 100));
	CHECK(libfaer_v0_23_GeneralizedHessenbergParams_f32().block_size == 32);
	CHECK(libfaer_v0_23_GeneralizedSchurParams_f64().nibble_threshold == libfaer_v0_23_SchurParams_f64().nibble_threshold);
	const FaerV0_24_Par seq = {FaerV0_24_ParTag_Seq, 0};
	const FaerV0_24_Layout l0 = libfaer_v0_23_generalized_evd_scratch_f64(0, FaerV0_24_ComputeEigenvectors_Yes, FaerV0_24_ComputeEigenvectors_Yes, seq, p);
	const FaerV0_24_Layout l1 = libfaer_v0_23_generalized_evd_scratch_f64(50, FaerV0_24_ComputeEigenvectors_No, FaerV0_24_ComputeEigenvectors_No, seq, p);
	const FaerV0_24_Layout l2 = libfaer_v0_23_generalized_evd_scratch_f64(50, FaerV0_24_ComputeEigenvectors_Yes, FaerV0_24_ComputeEigenvectors_Yes, seq, p);
	const FaerV0_24_Layout l3 = libfaer_v0_23_generalized_evd_scratch_f32(100, FaerV0_24_ComputeEigenvectors_Yes, FaerV0_24_ComputeEigenvectors_Yes, seq, q);
	CHECK(l0.len_bytes == 0 && l1.len_bytes > 0 && l2.len_bytes > l1.len_bytes && l3.len_bytes > 0);
	return 0;
}

#define N 12
static int compute(void)
{
	static double a[N * N], b[N * N], ur[N * N], alpha[N], alpha_im[N], beta[N];
	unsigned s = 12345u;
	double na = 0, nb = 0;
	for (int i = 0; i < N * N; ++i) {
		s = s * 1664525u + 1013904223u;
		a[i] = (double) (s >> 8) / (double) (1u << 24) - 0.5;
		s = s * 1664525u + 1013904223u;
		b[i] = (double) (s >> 8) / (double) (1u << 24) - 0.5 + (i % (N + 1) == 0 ? 2.0 : 0.0);
		na += a[i] * a[i];
		nb += b[i] * b[i];
	}
	na = sqrt(na);
	nb = sqrt(nb);
	const FaerV0_24_MatMut A = {a, N, N, 1, N}, B = {b, N, N, 1, N}, UR = {ur, N, N, 1, N}, UL = {NULL, N, 0, 1, N};
	const FaerV0_24_VecMut al = {alpha, N, 1}, ai = {alpha_im, N, 1}, be = {beta, N, 1};
	const FaerV0_24_Par seq = {FaerV0_24_ParTag_Seq, 0};
	const FaerV0_24_MemAlloc mem = {NULL, 0};
	const FaerV0_24_GevdStatus st = libfaer_v0_23_generalized_evd_f64(A, B, UL, UR, al, ai, be, seq, mem, libfaer_v0_23_GevdParams_f64());
	CHECK(st.tag == FaerV0_24_GevdStatus_Ok);
	for (int k = 0; k < N; ++k) {
		/* column k as a complex vector: real eigenvalue -> column k; a pair at (k, k + 1) -> real part, imaginary part */
		const double *xr, *xi;
		double sign = 1;
		if (alpha_im[k] == 0) {
			xr = ur + k * N;
			xi = NULL;
		} else if (alpha_im[k] > 0) {
			CHECK(k + 1 < N && alpha_im[k + 1] == -alpha_im[k]);
			xr = ur + k * N;
			xi = ur + (k + 1) * N;
		} else {
			xr = ur + (k - 1) * N;
			xi = ur + k * N;
			sign = -1;
		}
		double res = 0, nx = 0;
		for (int i = 0; i < N; ++i) {
			double axr = 0, axi = 0, bxr = 0, bxi = 0;
			for (int j = 0; j < N; ++j) {
				const double vr = xr[j], vi = xi ? sign * xi[j] : 0.0;
				axr += a[i + j * N] * vr;
				axi += a[i + j * N] * vi;
				bxr += b[i + j * N] * vr;
				bxi += b[i + j * N] * vi;
			}
			const double rr = beta[k] * axr - (alpha[k] * bxr - alpha_im[k] * bxi), ri = beta[k] * axi - (alpha[k] * bxi + alpha_im[k] * bxr);
			res += rr * rr + ri * ri;
			nx += xr[i] * xr[i] + (xi ? xi[i] * xi[i] : 0.0);
		}
		const double den = (fabs(beta[k]) * na + hypot(alpha[k], alpha_im[k]) * nb) * sqrt(nx);
		CHECK(nx > 0 && sqrt(res) <= 64 * N * 2.220446049250313e-16 * den);
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (host_only())
		return 1;
	if (argc > 1 && strcmp(argv[1], "compute") == 0) {
		if (faer_hip_device_count() < 1) {
			printf("no gfx950 device\n");
			return 2;
		}
		if (compute())
			return 1;
		printf("gevd_client ok (compute)\n");
		return 0;
	}
	printf("gevd_client ok (host-only)\n");
	return 0;
}
