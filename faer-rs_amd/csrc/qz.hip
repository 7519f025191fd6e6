// Generalized real eigendecomposition (gevd/mod.rs:130-320, gevd_real): QR of B, reduction of the pair to Hessenberg-triangular
// form, QZ iteration, eigenvectors of the quasi-triangular pair, two products.
//
// The arithmetic of every kernel is in qz_core.h (one body for the device and for a host compiler); this file holds the kernels
// around those bodies -- what they keep in LDS, what they load and store -- and the driver.
//
//   gevd_hess_tri_kernel  one workgroup: the rotations of the Hessenberg-triangular reduction, on global memory.
//   gevd_scan_kernel      one workgroup, global memory, between two sweeps: both deflation tests, the deflation of infinite
//                         eigenvalues, 1 x 1 and 2 x 2 blocks finished with their (alpha, beta), the next active block into the
//                         state record the host reads once per sweep.
//   gevd_leaf_kernel      one workgroup, a diagonal block of at most W rows of H and T and its two factors in LDS: the iteration to
//                         convergence.  Four (W + 1) x W matrices: W = 64 (fp64) / 96 (fp32), 133,120 / 148,992 bytes of the 160 KiB.
//   gevd_shift_kernel     the same iteration, eigenvalues only, on the trailing ns x ns sub-pencil: the shifts of a sweep.
//   gevd_window_kernel    one workgroup, a W x W window of H and T and two identities in LDS: a chain of ns / 2 bulges is
//                         introduced at the top of the active block, carried through the window or run off its bottom.
//   gevd_vec_kernel       one workgroup per eigenvalue (or pair): the shifted back substitution, column oriented.
//
// Per window step: one window launch, the copies and six products on gemm_dev (H and T right of the window, H and T above it,
// Q and Z).  Read-backs: the finite check, one per scan, the counters at the end.
#include "arena.h"
#include "qz_core.h"

namespace fh {

using namespace qz;

namespace {

struct DevGroup {
	__device__ int tid() const { return (int) threadIdx.x; }
	__device__ int size() const { return (int) blockDim.x; }
	__device__ void sync() const { __syncthreads(); }
};

constexpr int QZ_THREADS = 256;
template <typename T> constexpr idx_t qz_w() { return sizeof(T) == 8 ? 64 : 96; }
template <typename T> constexpr size_t qz_lds() { return 4 * (size_t) (qz_w<T>() + 1) * qz_w<T>() * sizeof(T); }

extern __shared__ __align__(16) unsigned char qz_smem[];

template <typename T> __device__ void qz_copy_block(T *dst, long ldd, const T *src, long lds_, long m)
{
	for (long e = threadIdx.x; e < m * m; e += blockDim.x) {
		const long i = e % m, j = e / m;
		dst[i + j * ldd] = src[i + j * lds_];
	}
}

template <typename T> __global__ __launch_bounds__(QZ_THREADS) void gevd_hess_tri_kernel(T *a, T *b, T *q, T *z, long n)
{
	hessenberg_triangular(DevGroup{}, Pencil<T>{a, n, b, n, n, q, n, z, n});
}

// norms[0], norms[1] <- Frobenius norms of h and t (n x n, dense), in a fixed order
template <typename T> __global__ __launch_bounds__(QZ_THREADS) void gevd_norms_kernel(const T *h, const T *t, long n, T *norms)
{
	__shared__ T part[2][QZ_THREADS];
	// scaled by the largest entry, so that the squares stay in range
	T mh = 0, mt = 0;
	for (long e = threadIdx.x; e < n * n; e += QZ_THREADS) {
		mh = sc_max(mh, sc_abs(h[e]));
		mt = sc_max(mt, sc_abs(t[e]));
	}
	part[0][threadIdx.x] = mh;
	part[1][threadIdx.x] = mt;
	__syncthreads();
	for (int w = QZ_THREADS / 2; w > 0; w >>= 1) {
		if ((int) threadIdx.x < w) {
			part[0][threadIdx.x] = sc_max(part[0][threadIdx.x], part[0][threadIdx.x + w]);
			part[1][threadIdx.x] = sc_max(part[1][threadIdx.x], part[1][threadIdx.x + w]);
		}
		__syncthreads();
	}
	mh = part[0][0];
	mt = part[1][0];
	__syncthreads();
	const T ih = mh > 0 ? 1 / mh : (T) 0, it = mt > 0 ? 1 / mt : (T) 0;
	T sh = 0, st = 0;
	for (long e = threadIdx.x; e < n * n; e += QZ_THREADS) {
		sh += (h[e] * ih) * (h[e] * ih);
		st += (t[e] * it) * (t[e] * it);
	}
	part[0][threadIdx.x] = sh;
	part[1][threadIdx.x] = st;
	__syncthreads();
	for (int w = QZ_THREADS / 2; w > 0; w >>= 1) {
		if ((int) threadIdx.x < w) {
			part[0][threadIdx.x] += part[0][threadIdx.x + w];
			part[1][threadIdx.x] += part[1][threadIdx.x + w];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		norms[0] = mh * sc_sqrt(part[0][0]);
		norms[1] = mt * sc_sqrt(part[1][0]);
	}
}

// state record beyond the counters of qz_core.h
enum { QS_ILO = 8, QS_IHI = 9, QS_DONE = 10 };

// LDS image (ld = W + 1) of the m x m diagonal block of the pair at global row w0, identities in the two accumulators
template <typename T> __device__ Pencil<T> qz_load_window(const T *h, const T *t, long n, long w0, long m, bool factors)
{
	constexpr long W = qz_w<T>(), LD = W + 1;
	T *lh = reinterpret_cast<T *>(qz_smem), *lt = lh + LD * W, *lu = lt + LD * W, *lv = lu + LD * W;
	qz_copy_block(lh, LD, h + w0 + w0 * n, n, m);
	qz_copy_block(lt, LD, t + w0 + w0 * n, n, m);
	if (factors)
		for (long e = threadIdx.x; e < m * m; e += blockDim.x) {
			const long i = e % m, j = e / m;
			lu[i + j * LD] = lv[i + j * LD] = i == j ? (T) 1 : (T) 0;
		}
	__syncthreads();
	return Pencil<T>{lh, LD, lt, LD, m, factors ? lu : (T *) nullptr, LD, factors ? lv : (T *) nullptr, LD};
}
template <typename T> __device__ void qz_store_window(const Pencil<T> &p, T *h, T *t, long n, long w0, T *u, T *v)
{
	__syncthreads();
	qz_copy_block(h + w0 + w0 * n, n, p.h, p.ldh, p.n);
	qz_copy_block(t + w0 + w0 * n, n, p.t, p.ldt, p.n);
	qz_copy_block(u, p.n, p.q, p.ldq, p.n);
	qz_copy_block(v, p.n, p.z, p.ldz, p.n);
}

// between two sweeps, on global memory: both deflation tests from row hi - 1 upwards, 1 x 1 and 2 x 2 blocks finished with their
// (alpha, beta), then the lowest block of three rows or more into the state record
template <typename T>
__global__ __launch_bounds__(QZ_THREADS) void gevd_scan_kernel(T *h, T *t, T *q, T *z, long n, long hi, T *ar, T *ai, T *be, const T *norms, long cap, int *st)
{
	long bf = 0, bl = 0;
	const long r = qz_unblocked(DevGroup{}, Pencil<T>{h, n, t, n, n, q, n, z, n}, ar, ai, be, norms[0], norms[1], cap, st, hi - 1, 3L, bf, bl);
	if (threadIdx.x == 0) {
		if (r > 0)
			st[QC_STATUS] = 1;
		st[QS_ILO] = (int) bf;
		st[QS_IHI] = (int) (bl + 1);
		st[QS_DONE] = r == 0;
	}
}

// the m x m diagonal block at row w0 (m <= W) in LDS: the iteration to convergence; u, v (m x m, dense) <- its two factors
template <typename T>
__global__ __launch_bounds__(QZ_THREADS) void gevd_leaf_kernel(T *h, T *t, long n, long w0, long m, T *ar, T *ai, T *be, const T *norms, long cap, T *u, T *v, int *st)
{
	const Pencil<T> p = qz_load_window(h, t, n, w0, m, true);
	long bf, bl;
	const long err = qz_unblocked(DevGroup{}, p, ar + w0, ai + w0, be + w0, norms[0], norms[1], cap, st, m - 1, 0L, bf, bl);
	if (threadIdx.x == 0 && err != 0)
		st[QC_STATUS] = 1;
	qz_store_window(p, h, t, n, w0, u, v);
}

// sr, si (ns entries) <- the shifts of the sweep on the active block that ends at row istop (exclusive)
template <typename T>
__global__ __launch_bounds__(QZ_THREADS) void gevd_shift_kernel(const T *h, const T *t, long n, long istop, int ns, int exceptional, const T *norms, long cap, T *sr, T *si)
{
	__shared__ T ev[5][qz_w<T>()];
	__shared__ int scratch[QC_COUNT];
	long err = 1, bf, bl;
	if (threadIdx.x < QC_COUNT)
		scratch[threadIdx.x] = 0;
	if (!exceptional) {
		const Pencil<T> p = qz_load_window(h, t, n, istop - ns, (long) ns, false);
		err = qz_unblocked(DevGroup{}, p, ev[0], ev[1], ev[2], norms[0], norms[1], cap, scratch, (long) ns - 1, 0L, bf, bl);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		qz_sweep_shifts(h, n, t, n, istop, ns, exceptional != 0, err, (const T *) ev[0], (const T *) ev[1], (const T *) ev[2], norms[0], norms[1], ev[3], ev[4]);
		for (int i = 0; i < ns; ++i) {
			sr[i] = ev[3][i];
			si[i] = ev[4][i];
		}
	}
}

// one window step: the ws x ws window at row w0 and two identities in LDS, a chain of nb bulges introduced, chased or run off
template <typename T>
__global__ __launch_bounds__(QZ_THREADS) void gevd_window_kernel(T *h, T *t, long n, long w0, long ws, long ilo, long ihi, int nb, const T *sr, const T *si, const T *norms,
								  long A, long B, T *u, T *v)
{
	__shared__ T ls[2][qz_w<T>()];
	for (int i = threadIdx.x; i < 2 * nb; i += blockDim.x) {
		ls[0][i] = sr[i];
		ls[1][i] = si[i];
	}
	const Pencil<T> p = qz_load_window(h, t, n, w0, ws, true);
	qz_window_chase(DevGroup{}, p, w0, ilo, ihi, nb, (const T *) ls[0], (const T *) ls[1], norms[0], norms[1], A, B);
	qz_store_window(p, h, t, n, w0, u, v);
}

template <typename T>
__global__ __launch_bounds__(QZ_THREADS) void gevd_vec_kernel(const T *sp, long srs, long scs, const T *pp, long prs, long pcs, long n, const T *ar, const T *ai,
							       const T *be, long es, T imsign, int swap, T *xp, long xrs, long xcs, const T *norms)
{
	gevec_block(DevGroup{}, sp, srs, scs, pp, prs, pcs, n, (long) blockIdx.x, ar, ai, be, es, imsign, swap != 0, xp, xrs, xcs, norms[0], norms[1]);
}

// st[QC_NONFINITE] <- 1 if the view holds an Inf or a NaN (gevd/mod.rs:225)
template <typename T> __global__ void gevd_nonfinite_kernel(const T *a, long rs, long cs, long nrows, long ncols, int *st)
{
	const long total = nrows * ncols;
	for (long e = blockIdx.x * (long) blockDim.x + threadIdx.x; e < total; e += (long) gridDim.x * blockDim.x) {
		const T v = a[(e % nrows) * rs + (e / nrows) * cs];
		if (!(sc_abs(v) <= (sizeof(T) == 8 ? (T) DBL_MAX : (T) FLT_MAX))) // (false for a NaN as well)
			st[QC_NONFINITE] = 1;
	}
}

// the reflectors below the diagonal leave (gevd/mod.rs:280-284)
template <typename T> __global__ void gevd_clear_lower_kernel(T *b, long ld, long n)
{
	const long total = n * n;
	for (long e = blockIdx.x * (long) blockDim.x + threadIdx.x; e < total; e += (long) gridDim.x * blockDim.x) {
		const long i = e % n, j = e / n;
		if (i > j)
			b[i + j * ld] = 0;
	}
}

unsigned gevd_grid(long total)
{
	long b = (total + 255) / 256;
	return (unsigned) (b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// the device backend of qz_drive (qz_core.h)
template <typename T> struct DeviceQz {
	MatV<T> H, Tm, Q, Z; // Q.p == nullptr: no vectors
	T *ar, *ai, *be, *norms, *sr, *si, *u, *v, *tmp;
	int *st;
	hipStream_t s;
	idx_t n;
	long cap;

	void read_state(int *out)
	{
		int *pin = ctx().pinned_ints();
		FH_HIP(hipMemcpyAsync(pin, st, QC_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
		memcpy(out, pin, QC_COUNT * sizeof(int));
	}
	bool scan(long hi, long &ilo, long &ihi, bool &done)
	{
		hipLaunchKernelGGL(gevd_scan_kernel<T>, dim3(1), dim3(QZ_THREADS), 0, s, H.p, Tm.p, Q.p, Z.p, n, hi, ar, ai, be, (const T *) norms, cap, st);
		FH_HIP(hipGetLastError());
		int v_[QC_COUNT];
		read_state(v_);
		ilo = v_[QS_ILO];
		ihi = v_[QS_IHI];
		done = v_[QS_DONE] != 0;
		return v_[QC_STATUS] == 0;
	}
	// the pair and its factors outside the diagonal block [w0, w0 + ws) take the block's two factors u, v (ws x ws, dense)
	void off_block(idx_t w0, idx_t ws)
	{
		const MatV<const T> U{u, ws, ws, 1, ws}, V{v, ws, ws, 1, ws};
		const idx_t right = n - (w0 + ws);
		for (MatV<T> M : {H, Tm}) {
			if (right > 0) {
				MatV<T> dst = M.sub(w0, w0 + ws, ws, right), t{tmp, ws, right, 1, ws};
				copy_dev<T>(t, dst.c());
				gemm_dev<T>(dst, DST_FULL, false, U.t(), t.c(), (T) 1);
			}
			if (w0 > 0) {
				MatV<T> dst = M.sub(0, w0, w0, ws), t{tmp, w0, ws, 1, w0};
				copy_dev<T>(t, dst.c());
				gemm_dev<T>(dst, DST_FULL, false, t.c(), V, (T) 1);
			}
		}
		if (Q.p) {
			MatV<T> t{tmp, n, ws, 1, n}, dq = Q.sub(0, w0, n, ws), dz = Z.sub(0, w0, n, ws);
			copy_dev<T>(t, dq.c());
			gemm_dev<T>(dq, DST_FULL, false, t.c(), U, (T) 1);
			copy_dev<T>(t, dz.c());
			gemm_dev<T>(dz, DST_FULL, false, t.c(), V, (T) 1);
		}
	}
	void leaf(long ilo, long m)
	{
		hipLaunchKernelGGL(gevd_leaf_kernel<T>, dim3(1), dim3(QZ_THREADS), qz_lds<T>(), s, H.p, Tm.p, n, ilo, m, ar, ai, be, (const T *) norms, cap, u, v, st);
		FH_HIP(hipGetLastError());
		off_block((idx_t) ilo, (idx_t) m); // (the leaf's own status is in the state record: the next scan reports it)
	}
	void shifts(long, long ihi, int ns, bool exceptional)
	{
		hipLaunchKernelGGL(gevd_shift_kernel<T>, dim3(1), dim3(QZ_THREADS), qz_lds<T>(), s, (const T *) H.p, (const T *) Tm.p, n, ihi, ns, exceptional ? 1 : 0,
				   (const T *) norms, cap, sr, si);
		FH_HIP(hipGetLastError());
	}
	void window(long w0, long ws, long ilo, long ihi, int nb, long A, long B)
	{
		hipLaunchKernelGGL(gevd_window_kernel<T>, dim3(1), dim3(QZ_THREADS), qz_lds<T>(), s, H.p, Tm.p, n, w0, ws, ilo, ihi, nb, (const T *) sr, (const T *) si, (const T *) norms, A,
				   B, u, v);
		FH_HIP(hipGetLastError());
		off_block((idx_t) w0, (idx_t) ws);
	}
};

thread_local long g_gevd_counts[5] = {0, 0, 0, 0, 0};

} // namespace

idx_t gevd_window_edge(int elem_bytes) { return elem_bytes == 8 ? qz_w<double>() : qz_w<float>(); }
void gevd_last_counts(long out[5]) { memcpy(out, g_gevd_counts, sizeof(g_gevd_counts)); }

// bytes of the arena of one call (gevd_dev carves exactly these slices; the staging slices of host operands come on top)
size_t gevd_arena_bytes(idx_t n, bool vectors, idx_t bs, int elem_bytes)
{
	const size_t N = (size_t) n, e = (size_t) elem_bytes;
	auto pad = [](size_t b) { return Arena::padded(b); };
	const size_t W = (size_t) gevd_window_edge(elem_bytes);
	size_t total = pad(QC_COUNT * sizeof(int)) + 2 * pad(N * N * e) + pad((size_t) bs * N * e) + pad(2 * e) + pad(N * W * e) + 2 * pad(W * W * e) + 2 * pad(W * e);
	if (vectors)
		total += 3 * pad(N * N * e);
	return total;
}

// A, B: n x n, never written.  alpha_re / alpha_im / beta: n contiguous device entries.  UL / UR: n x n or .p == nullptr.
// Returns 0, or 1 for NoConvergence (a non-finite entry, or the iteration cap).
template <typename T>
int gevd_dev(Arena &ar, MatV<const T> A, MatV<const T> B, MatV<T> UL, MatV<T> UR, T *alpha_re, T *alpha_im, T *beta, idx_t bs, idx_t qr_blocking_threshold,
	     size_t (*shift_count)(size_t, size_t))
{
	const idx_t n = A.nrows;
	FH_CHECK(n > 0 && n < (1L << 30), "generalized_evd: matrix too large");
	hipStream_t s = ctx().stream;
	const bool vectors = UL.p != nullptr || UR.p != nullptr;
	constexpr idx_t W = qz_w<T>();
	int *st = ar.take<int>(QC_COUNT);
	FH_HIP(hipMemsetAsync(st, 0, QC_COUNT * sizeof(int), s));
	hipLaunchKernelGGL(gevd_nonfinite_kernel<T>, dim3(gevd_grid(n * n)), dim3(256), 0, s, A.p, A.rs, A.cs, n, n, st);
	hipLaunchKernelGGL(gevd_nonfinite_kernel<T>, dim3(gevd_grid(n * n)), dim3(256), 0, s, B.p, B.rs, B.cs, n, n, st);
	FH_HIP(hipGetLastError());
	long readbacks = 0;
	auto read_state = [&](int *out) {
		int *pin = ctx().pinned_ints();
		FH_HIP(hipMemcpyAsync(pin, st, QC_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
		memcpy(out, pin, QC_COUNT * sizeof(int));
		++readbacks;
	};
	int v[QC_COUNT];
	read_state(v);
	memset(g_gevd_counts, 0, sizeof(g_gevd_counts));
	g_gevd_counts[3] = readbacks;
	if (v[QC_NONFINITE])
		return 1;
	// stage 0 (gevd/mod.rs:249-284): B = Q R, A <- Q^T A, UL <- Q
	MatV<T> H = ar.mat<T>(n, n), Tm = ar.mat<T>(n, n);
	copy_dev<T>(H, A);
	copy_dev<T>(Tm, B);
	MatV<T> Hh{ar.take<T>((size_t) bs * (size_t) n), bs, n, 1, bs};
	T *norms = ar.take<T>(2);
	MatV<T> Q{nullptr, n, n, 1, n}, Z{nullptr, n, n, 1, n}, X{nullptr, n, n, 1, n};
	if (vectors) {
		Q = ar.mat<T>(n, n);
		Z = ar.mat<T>(n, n);
		X = ar.mat<T>(n, n);
		svd_identity_dev<T>(Q);
		svd_identity_dev<T>(Z);
	}
	geqrf_dev<T>(Tm, Hh, qr_blocking_threshold);
	apply_householder_sequence_left_dev<T>(Tm.c(), Hh.c(), H, true);
	if (vectors)
		apply_householder_sequence_left_dev<T>(Tm.c(), Hh.c(), Q, false);
	hipLaunchKernelGGL(gevd_clear_lower_kernel<T>, dim3(gevd_grid(n * n)), dim3(256), 0, s, Tm.p, Tm.cs, n);
	// stage 1
	hipLaunchKernelGGL(gevd_hess_tri_kernel<T>, dim3(1), dim3(QZ_THREADS), 0, s, H.p, Tm.p, Q.p, Z.p, n);
	// stage 2
	hipLaunchKernelGGL(gevd_norms_kernel<T>, dim3(1), dim3(QZ_THREADS), 0, s, (const T *) H.p, (const T *) Tm.p, n, norms);
	DeviceQz<T> be;
	be.H = H;
	be.Tm = Tm;
	be.Q = Q;
	be.Z = Z;
	be.ar = alpha_re;
	be.ai = alpha_im;
	be.be = beta;
	be.norms = norms;
	be.tmp = ar.take<T>((size_t) n * (size_t) W);
	be.u = ar.take<T>((size_t) W * (size_t) W);
	be.v = ar.take<T>((size_t) W * (size_t) W);
	be.sr = ar.take<T>((size_t) W);
	be.si = ar.take<T>((size_t) W);
	be.st = st;
	be.s = s;
	be.n = n;
	be.cap = 30 * (n > 10 ? n : 10);
	raise_dynamic_lds<&gevd_leaf_kernel<T>>(qz_lds<T>());
	raise_dynamic_lds<&gevd_shift_kernel<T>>(qz_lds<T>());
	raise_dynamic_lds<&gevd_window_kernel<T>>(qz_lds<T>());
	GevdCounts cnt;
	const int r = qz_drive(be, (long) n, (long) W, shift_count, cnt);
	read_state(v); // the counters of the kernels
	g_gevd_counts[0] = cnt.sweeps;
	g_gevd_counts[1] = cnt.window_steps;
	g_gevd_counts[2] = cnt.leaves;
	g_gevd_counts[3] = readbacks + cnt.readbacks;
	g_gevd_counts[4] = v[QC_INFINITE];
	if (r != 0 || v[QC_STATUS] != 0)
		return 1;
	// stage 3: UR = Z X, UL = Q Y
	if (UR.p) {
		hipLaunchKernelGGL(gevd_vec_kernel<T>, dim3((unsigned) n), dim3(QZ_THREADS), 0, s, (const T *) H.p, H.rs, H.cs, (const T *) Tm.p, Tm.rs, Tm.cs, n,
				   (const T *) alpha_re, (const T *) alpha_im, (const T *) beta, 1L, (T) 1, 0, X.p, X.rs, X.cs, (const T *) norms);
		FH_HIP(hipGetLastError());
		gemm_dev<T>(UR, DST_FULL, false, Z.c(), X.c(), (T) 1);
	}
	if (UL.p) {
		// the same solve on the transposed pair with rows and columns reversed; X is written through the reversed view as well
		const MatV<T> Sv = H.t().rev_rows().rev_cols(), Pv = Tm.t().rev_rows().rev_cols(), Xv = X.rev_rows().rev_cols();
		hipLaunchKernelGGL(gevd_vec_kernel<T>, dim3((unsigned) n), dim3(QZ_THREADS), 0, s, (const T *) Sv.p, Sv.rs, Sv.cs, (const T *) Pv.p, Pv.rs, Pv.cs, n,
				   (const T *) alpha_re + (n - 1), (const T *) alpha_im + (n - 1), (const T *) beta + (n - 1), -1L, (T) -1, 1, Xv.p, Xv.rs, Xv.cs,
				   (const T *) norms);
		FH_HIP(hipGetLastError());
		gemm_dev<T>(UL, DST_FULL, false, Q.c(), X.c(), (T) 1);
	}
	FH_HIP(hipStreamSynchronize(s)); // the arena goes back to the pool when the caller returns
	return 0;
}

template int gevd_dev<double>(Arena &, MatV<const double>, MatV<const double>, MatV<double>, MatV<double>, double *, double *, double *, idx_t, idx_t, size_t (*)(size_t, size_t));
template int gevd_dev<float>(Arena &, MatV<const float>, MatV<const float>, MatV<float>, MatV<float>, float *, float *, float *, idx_t, idx_t, size_t (*)(size_t, size_t));

} // namespace fh
