// General real eigendecomposition (evd/mod.rs:1007-1174, evd_imp): Hessenberg reduction (condense.hip), real Schur form
// by multishift QR sweeps, eigenvectors of the quasi-triangular factor, two triangular products.
//
// The arithmetic of every kernel is in schur_core.h (one body for the device and for a host compiler); this file holds the
// kernels around those bodies -- what they keep in LDS, what they load and store -- and the driver.
//
//   schur_leaf_kernel    one workgroup, a diagonal block of at most W rows and its orthogonal factor in LDS: lahqr to
//                        convergence.  The whole problem for n <= W, the clean-up of every active block once it is <= W.
//   schur_shift_kernel   the same iteration, eigenvalues only, on the LDS image of the trailing ns x ns block: the shifts
//                        of a sweep (the matrix in global memory is not touched).
//   schur_window_kernel  one workgroup, a W x W diagonal window of H and a W x W identity in LDS: a chain of ns / 2 bulges
//                        is introduced at the top of the active block, carried through the window or run off its bottom.
//   schur_prepare_kernel the classical deflation test on the whole subdiagonal and the next active block, into the state
//                        record the host reads once per sweep.
//   schur_finish_kernel  standard form of the 2 x 2 blocks the sweeps isolated, (w_re, w_im).
//   eigvec_kernel        one workgroup per eigenvalue (or pair): the shifted back substitution, column oriented.
//
// Per window step: one window launch, then three copies and three products on gemm_dev for the parts of H and Z outside
// the window.  W = 96 (fp64) / 128 (fp32): two (W + 1) x W matrices and 2 W shift slots, 150,528 / 133,120 bytes of the 160 KiB.
#include "arena.h"
#include "schur_core.h"

namespace fh {

using namespace schur;

namespace {

struct DevGroup {
	__device__ int tid() const { return (int) threadIdx.x; }
	__device__ int size() const { return (int) blockDim.x; }
	__device__ void sync() const { __syncthreads(); }
	__device__ void atomic_max(int *p, int v) const { atomicMax(p, v); }
	__device__ void atomic_add(int *p, int v) const { atomicAdd(p, v); }
};

constexpr int SCHUR_THREADS = 256;
template <typename T> constexpr idx_t schur_w() { return sizeof(T) == 8 ? 96 : 128; }
template <typename T> constexpr size_t schur_lds() { return (2 * (size_t) (schur_w<T>() + 1) * schur_w<T>() + 2 * schur_w<T>()) * sizeof(T); }

extern __shared__ __align__(16) unsigned char schur_smem[];

// LDS image (ld = W + 1) of the m x m block at h, nothing below the subdiagonal
template <typename T> __device__ void load_hessenberg(T *a, long lda, const T *h, long ld, long m)
{
	for (long e = threadIdx.x; e < m * m; e += blockDim.x) {
		const long i = e % m, j = e / m;
		a[i + j * lda] = i <= j + 1 ? h[i + j * ld] : (T) 0;
	}
}
template <typename T> __device__ void load_identity(T *q, long ldq, long m)
{
	for (long e = threadIdx.x; e < m * m; e += blockDim.x) {
		const long i = e % m, j = e / m;
		q[i + j * ldq] = i == j ? (T) 1 : (T) 0;
	}
}
template <typename T> __device__ void store_block(T *dst, long ld, const T *a, long lda, long m)
{
	for (long e = threadIdx.x; e < m * m; e += blockDim.x) {
		const long i = e % m, j = e / m;
		dst[i + j * ld] = a[i + j * lda];
	}
}

template <typename T>
__global__ __launch_bounds__(SCHUR_THREADS) void schur_leaf_kernel(T *h, long ld, long m, T *q, T *wr, T *wi, int *st)
{
	constexpr long W = schur_w<T>(), LD = W + 1;
	T *a = reinterpret_cast<T *>(schur_smem), *z = a + LD * W;
	load_hessenberg(a, LD, h, ld, m);
	load_identity(z, LD, m);
	__syncthreads();
	const long err = lahqr(DevGroup{}, true, a, LD, m, z, LD, wr, wi);
	__syncthreads();
	if (err != 0) { // h stays as it was and q is the identity: what follows until the next read-back changes nothing
		if (threadIdx.x == 0)
			st[ST_STATUS] = 1;
		load_identity(q, m, m);
		return;
	}
	store_block(h, ld, a, LD, m);
	store_block(q, m, z, LD, m);
}

// sr, si (ns entries) <- the shifts of the sweep on the active block that ends at row istop of h (n x n)
template <typename T>
__global__ __launch_bounds__(SCHUR_THREADS) void schur_shift_kernel(const T *h, long ld, long istop, int ns, int exceptional, T *sr, T *si, int *st)
{
	constexpr long W = schur_w<T>(), LD = W + 1;
	T *a = reinterpret_cast<T *>(schur_smem), *wr = a + 2 * LD * W, *wi = wr + W;
	long err = exceptional;
	if (!exceptional) {
		const long o = istop - ns;
		load_hessenberg(a, LD, h + o + o * ld, ld, (long) ns);
		__syncthreads();
		err = lahqr(DevGroup{}, false, a, LD, (long) ns, (T *) nullptr, 0L, wr, wi);
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		if (err != 0) {
			exceptional_shifts(h, ld, istop, ns, wr, wi);
			if (!exceptional)
				st[ST_SHIFT_ERR] += 1;
		}
		pair_shifts(wr, wi, ns, h[(istop - 1) + (istop - 1) * ld]);
		for (int i = 0; i < ns; ++i) {
			sr[i] = wr[i];
			si[i] = wi[i];
		}
	}
}

template <typename T>
__global__ __launch_bounds__(SCHUR_THREADS) void schur_window_kernel(T *h, long ld, long w0, long ws, long ilo, long ihi, int nb, const T *sr, const T *si,
								      long A, long B, T *u)
{
	constexpr long W = schur_w<T>(), LD = W + 1;
	T *a = reinterpret_cast<T *>(schur_smem), *z = a + LD * W, *lr = a + 2 * LD * W, *li = lr + W;
	T *hw = h + w0 + w0 * ld;
	for (long e = threadIdx.x; e < ws * ws; e += blockDim.x) {
		const long i = e % ws, j = e / ws;
		a[i + j * LD] = hw[i + j * ld];
	}
	load_identity(z, LD, ws);
	for (int i = threadIdx.x; i < 2 * nb; i += blockDim.x) {
		lr[i] = sr[i];
		li[i] = si[i];
	}
	__syncthreads();
	window_chase(DevGroup{}, a, LD, z, LD, ws, w0, ilo, ihi, nb, lr, li, A, B);
	store_block(hw, ld, a, LD, ws);
	store_block(u, ws, z, LD, ws);
}

template <typename T> __global__ __launch_bounds__(SCHUR_THREADS) void schur_prepare_kernel(T *h, long ld, long n, long hi, int *st)
{
	__shared__ int red[3];
	sweep_prepare(DevGroup{}, h, ld, n, hi, st, red);
}

template <typename T> __global__ __launch_bounds__(SCHUR_THREADS) void schur_finish_kernel(T *h, long ld, long n, T *z, long ldz, T *wr, T *wi)
{
	schur_finish(DevGroup{}, h, ld, n, z, ldz, wr, wi);
}

template <typename T>
__global__ __launch_bounds__(SCHUR_THREADS) void eigvec_kernel(const T *tp, long trs, long tcs, long n, T *xp, long xrs, long xcs, const T *norm)
{
	eigvec_block(DevGroup{}, tp, trs, tcs, n, (long) blockIdx.x, xp, xrs, xcs, *norm);
}

// colsum[j] <- sum of |h(i, j)| over the Hessenberg part of column j; then norm <- their sum, both in a fixed order
template <typename T> __global__ __launch_bounds__(64) void hess_colsum_kernel(const T *h, long ld, long n, T *colsum)
{
	__shared__ T part[64];
	const long j = blockIdx.x, rows = j + 2 < n ? j + 2 : n;
	T s = 0;
	for (long i = threadIdx.x; i < rows; i += 64)
		s += sc_abs(h[i + j * ld]);
	part[threadIdx.x] = s;
	__syncthreads();
	for (int w = 32; w > 0; w >>= 1) {
		if ((int) threadIdx.x < w)
			part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		colsum[j] = part[0];
}
template <typename T> __global__ __launch_bounds__(SCHUR_THREADS) void hess_norm_kernel(const T *colsum, long n, T *norm)
{
	__shared__ T part[SCHUR_THREADS];
	T s = 0;
	for (long i = threadIdx.x; i < n; i += SCHUR_THREADS)
		s += colsum[i];
	part[threadIdx.x] = s;
	__syncthreads();
	for (int w = SCHUR_THREADS / 2; w > 0; w >>= 1) {
		if ((int) threadIdx.x < w)
			part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		*norm = part[0];
}

// st[ST_NONFINITE] <- 1 if the view holds an Inf or a NaN (evd/mod.rs:1021-1027)
template <typename T> __global__ void nonfinite_kernel(const T *a, long rs, long cs, long nrows, long ncols, int *st)
{
	const long total = nrows * ncols;
	for (long e = blockIdx.x * (long) blockDim.x + threadIdx.x; e < total; e += (long) gridDim.x * blockDim.x) {
		const T v = a[(e % nrows) * rs + (e / nrows) * cs];
		if (!(sc_abs(v) <= (sizeof(T) == 8 ? (T) DBL_MAX : (T) FLT_MAX))) // (false for a NaN as well)
			st[ST_NONFINITE] = 1;
	}
}

// the reflectors below the subdiagonal leave (evd/mod.rs:1076-1080)
template <typename T> __global__ void clear_below_subdiag_kernel(T *h, long ld, long n)
{
	const long total = n * n;
	for (long e = blockIdx.x * (long) blockDim.x + threadIdx.x; e < total; e += (long) gridDim.x * blockDim.x) {
		const long i = e % n, j = e / n;
		if (i > j + 1)
			h[i + j * ld] = 0;
	}
}

unsigned grid_for(long total)
{
	long b = (total + 255) / 256;
	return (unsigned) (b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// the device backend of schur_drive (schur_core.h)
template <typename T> struct DeviceSchur {
	static constexpr idx_t W = schur_w<T>();
	MatV<T> H, Z; // Z.p == nullptr: no vectors
	T *wr, *wi, *sr, *si, *u, *tmp;
	int *st;
	hipStream_t s;
	idx_t n;

	void read_state(int *out)
	{
		int *pin = ctx().pinned_ints();
		FH_HIP(hipMemcpyAsync(pin, st, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
		memcpy(out, pin, ST_COUNT * sizeof(int));
	}
	bool prepare(long hi, long &ilo, long &ihi, bool &done, long &deflated)
	{
		hipLaunchKernelGGL(schur_prepare_kernel<T>, dim3(1), dim3(SCHUR_THREADS), 0, s, H.p, H.cs, n, hi, st);
		FH_HIP(hipGetLastError());
		int v[ST_COUNT];
		read_state(v);
		ilo = v[ST_ILO];
		ihi = v[ST_IHI];
		done = v[ST_DONE] != 0;
		deflated = v[ST_DEFLATED];
		return v[ST_STATUS] == 0; // (set by a leaf over its iteration cap)
	}
	// H and Z outside the diagonal block [w0, w0 + ws) take the block's orthogonal factor q (ws x ws, dense)
	void off_block(idx_t w0, idx_t ws, T *q)
	{
		MatV<const T> Q{q, ws, ws, 1, ws};
		const idx_t right = n - (w0 + ws);
		if (right > 0) {
			MatV<T> dst = H.sub(w0, w0 + ws, ws, right), t{tmp, ws, right, 1, ws};
			copy_dev<T>(t, dst.c());
			gemm_dev<T>(dst, DST_FULL, false, Q.t(), t.c(), (T) 1);
		}
		if (w0 > 0) {
			MatV<T> dst = H.sub(0, w0, w0, ws), t{tmp, w0, ws, 1, w0};
			copy_dev<T>(t, dst.c());
			gemm_dev<T>(dst, DST_FULL, false, t.c(), Q, (T) 1);
		}
		if (Z.p) {
			MatV<T> dst = Z.sub(0, w0, n, ws), t{tmp, n, ws, 1, n};
			copy_dev<T>(t, dst.c());
			gemm_dev<T>(dst, DST_FULL, false, t.c(), Q, (T) 1);
		}
	}
	bool leaf(long ilo, long m)
	{
		hipLaunchKernelGGL(schur_leaf_kernel<T>, dim3(1), dim3(SCHUR_THREADS), schur_lds<T>(), s, H.p + ilo + ilo * H.cs, H.cs, m, u, wr + ilo, wi + ilo, st);
		FH_HIP(hipGetLastError());
		off_block((idx_t) ilo, (idx_t) m, u);
		return true; // the leaf's own status is in the state record: the next prepare reports it
	}
	void shifts(long, long ihi, int ns, bool exceptional)
	{
		hipLaunchKernelGGL(schur_shift_kernel<T>, dim3(1), dim3(SCHUR_THREADS), schur_lds<T>(), s, (const T *) H.p, H.cs, ihi, ns, exceptional ? 1 : 0, sr, si, st);
		FH_HIP(hipGetLastError());
	}
	void window(long w0, long ws, long ilo, long ihi, int nb, long A, long B)
	{
		hipLaunchKernelGGL(schur_window_kernel<T>, dim3(1), dim3(SCHUR_THREADS), schur_lds<T>(), s, H.p, H.cs, w0, ws, ilo, ihi, nb, (const T *) sr,
				   (const T *) si, A, B, u);
		FH_HIP(hipGetLastError());
		off_block((idx_t) w0, (idx_t) ws, u);
	}
	void finish()
	{
		hipLaunchKernelGGL(schur_finish_kernel<T>, dim3(1), dim3(SCHUR_THREADS), 0, s, H.p, H.cs, n, Z.p, Z.p ? Z.cs : 0, wr, wi);
		FH_HIP(hipGetLastError());
	}
};

thread_local long g_last_counts[4] = {0, 0, 0, 0};

} // namespace

idx_t schur_window_edge(int elem_bytes) { return elem_bytes == 8 ? schur_w<double>() : schur_w<float>(); }
void evd_last_counts(long out[4]) { memcpy(out, g_last_counts, sizeof(g_last_counts)); }

// bytes of the arena of one call (evd_dev carves exactly these slices; the staging slices of host operands come on top)
size_t evd_arena_bytes(idx_t n, bool vectors, idx_t bs, int elem_bytes)
{
	const size_t W = (size_t) schur_window_edge(elem_bytes), N = (size_t) n, e = (size_t) elem_bytes;
	auto pad = [](size_t b) { return Arena::padded(b); };
	size_t total = pad(N * N * e) + pad((size_t) bs * (N > 1 ? N - 1 : 1) * e) + pad(N * W * e) + pad(W * W * e) + 4 * pad(N * e) + 2 * pad(W * e)
		       + pad(ST_COUNT * sizeof(int)) + pad(e);
	if (vectors)
		total += 2 * pad(N * N * e);
	return total;
}

// evd/mod.rs:1007 evd_imp for a real matrix, all operands in device memory.  A: n x n, never written.  wr / wi: n
// contiguous device entries.  UL / UR: n x n or .p == nullptr.  Returns 0, or 1 for NoConvergence.
template <typename T>
int evd_dev(Arena &ar, MatV<const T> A, bool a_is_arena_dense, MatV<T> UL, MatV<T> UR, T *wr, T *wi, idx_t bs, size_t (*shift_count)(size_t, size_t))
{
	const idx_t n = A.nrows;
	FH_CHECK(n > 0 && n < (1L << 30), "evd: matrix too large");
	hipStream_t s = ctx().stream;
	const bool vectors = UL.p != nullptr || UR.p != nullptr;
	constexpr idx_t W = schur_w<T>();
	int *st = ar.take<int>(ST_COUNT);
	FH_HIP(hipMemsetAsync(st, 0, ST_COUNT * sizeof(int), s));
	hipLaunchKernelGGL(nonfinite_kernel<T>, dim3(grid_for(n * n)), dim3(256), 0, s, A.p, A.rs, A.cs, n, n, st);
	FH_HIP(hipGetLastError());
	DeviceSchur<T> be;
	be.st = st;
	be.s = s;
	be.n = n;
	{
		int v[ST_COUNT];
		be.read_state(v);
		if (v[ST_NONFINITE])
			return 1;
	}
	MatV<T> H;
	if (a_is_arena_dense)
		H = MatV<T>{const_cast<T *>(A.p), n, n, 1, n};
	else {
		H = ar.mat<T>(n, n);
		copy_dev<T>(H, A);
	}
	MatV<T> Hh{ar.take<T>((size_t) bs * (size_t) (n > 1 ? n - 1 : 1)), bs, n - 1, 1, bs};
	MatV<T> Z{nullptr, n, n, 1, n}, X{nullptr, n, n, 1, n};
	if (vectors) {
		Z = ar.mat<T>(n, n);
		X = ar.mat<T>(n, n);
		svd_identity_dev<T>(Z);
	}
	be.tmp = ar.take<T>((size_t) n * (size_t) W);
	be.u = ar.take<T>((size_t) W * (size_t) W);
	be.wr = wr;
	be.wi = wi;
	be.sr = ar.take<T>((size_t) W);
	be.si = ar.take<T>((size_t) W);
	T *colsum = ar.take<T>((size_t) n), *norm = ar.take<T>(1);
	if (n > 1) {
		hessenberg_dev<T>(H, Hh);
		if (vectors && n > 1)
			apply_householder_sequence_left_dev<T>(H.sub(1, 0, n - 1, n - 1).c(), Hh.c(), Z.sub(1, 1, n - 1, n - 1), false);
		hipLaunchKernelGGL(clear_below_subdiag_kernel<T>, dim3(grid_for(n * n)), dim3(256), 0, s, H.p, H.cs, n);
		FH_HIP(hipGetLastError());
	}
	be.H = H;
	be.Z = Z;
	raise_dynamic_lds<&schur_leaf_kernel<T>>(schur_lds<T>());
	raise_dynamic_lds<&schur_shift_kernel<T>>(schur_lds<T>());
	raise_dynamic_lds<&schur_window_kernel<T>>(schur_lds<T>());
	SchurCounts cnt;
	int r = schur_drive(be, (long) n, (long) W, shift_count, cnt);
	g_last_counts[0] = cnt.sweeps;
	g_last_counts[1] = cnt.window_steps;
	g_last_counts[2] = cnt.leaves;
	g_last_counts[3] = cnt.prepares;
	if (r != 0) {
		FH_HIP(hipStreamSynchronize(s));
		return 1;
	}
	if (vectors) {
		hipLaunchKernelGGL(hess_colsum_kernel<T>, dim3((unsigned) n), dim3(64), 0, s, (const T *) H.p, H.cs, n, colsum);
		hipLaunchKernelGGL(hess_norm_kernel<T>, dim3(1), dim3(SCHUR_THREADS), 0, s, (const T *) colsum, n, norm);
		FH_HIP(hipGetLastError());
	}
	if (UR.p) {
		hipLaunchKernelGGL(eigvec_kernel<T>, dim3((unsigned) n), dim3(SCHUR_THREADS), 0, s, (const T *) H.p, H.rs, H.cs, n, X.p, X.rs, X.cs, (const T *) norm);
		FH_HIP(hipGetLastError());
		matmul_triangular_dev<T>(UR, FaerBlock_Rectangular, false, Z.c(), FaerBlock_Rectangular, X.c(), FaerBlock_TriangularUpper, (T) 1);
	}
	if (UL.p) {
		// the same solve on the transposed, row- and column-reversed view; X is written through the reversed view as well, so
		// that it holds the lower triangular factor itself (evd/mod.rs:1140-1172)
		const MatV<T> Tv = H.t().rev_rows().rev_cols(), Xv = X.rev_rows().rev_cols();
		hipLaunchKernelGGL(eigvec_kernel<T>, dim3((unsigned) n), dim3(SCHUR_THREADS), 0, s, (const T *) Tv.p, Tv.rs, Tv.cs, n, Xv.p, Xv.rs, Xv.cs, (const T *) norm);
		FH_HIP(hipGetLastError());
		matmul_triangular_dev<T>(UL, FaerBlock_Rectangular, false, Z.c(), FaerBlock_Rectangular, X.c(), FaerBlock_TriangularLower, (T) 1);
	}
	FH_HIP(hipStreamSynchronize(s)); // the arena goes back to the pool when the caller returns
	return 0;
}

template int evd_dev<double>(Arena &, MatV<const double>, bool, MatV<double>, MatV<double>, double *, double *, idx_t, size_t (*)(size_t, size_t));
template int evd_dev<float>(Arena &, MatV<const float>, bool, MatV<float>, MatV<float>, float *, float *, idx_t, size_t (*)(size_t, size_t));

} // namespace fh
