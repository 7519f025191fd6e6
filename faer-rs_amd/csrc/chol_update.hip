// Modifying an existing Cholesky factorization on the device: rank-r update / downdate of L L^T and of L D L^T, and the deletion of
// rows and columns from L D L^T (cholesky/llt/update.rs:360, cholesky/ldlt/update.rs:376 and :417).  DESIGN.md section 3.15.
//
// The columns are walked in blocks of NB; a block takes two launches per chunk of at most RC columns of W:
//   diag_kernel  one wave.  The NB x NB diagonal block, its rows of the chunk and alpha live in LDS, lane i owns row i.  Column by
//                column every lane forms the coefficients (p', beta, gamma) redundantly and the lanes below the column apply
//                them; lane 0 writes the coefficient table.  This is the serial chain of the call.
//   tail_kernel  one row per lane for the rows below the block, its chunk of W in registers, the table in LDS; streams the block
//                column of L once.
// Nothing between the first and the last launch waits on the host.  A failing LLT pivot is recorded in a device status word
// (smallest failing column + 1); once it is set the tail kernels return at entry and a diagonal kernel runs only the columns in
// front of it (a later chunk may still fail at a smaller column: that is the index the reference reports).  The bodies are in
// chol_update_core.h, which tests/host/chol_update_host.cpp runs on the host.
#include "arena.h"
#include "chol_update_core.h"
#include "common.h"

namespace fh {

namespace {

using namespace cholup;

constexpr int CU_NB = 64;  // columns per block: one row of the diagonal block per lane of a wave
constexpr int CU_RC = 32;  // columns of W per chunk
constexpr int CU_TAIL_NT = 128;

thread_local long g_last[4] = {0, 0, 0, 0}; // column blocks, tail launches, chunks of W per block, host synchronisations inside the block loop
thread_local bool g_in_block_loop = false;
std::atomic<int> g_diag_only{0}; // measurement aid (tools/bench_chol_update.py): 1 = the tail launches are left out, the result is wrong

void sync_stream()
{
	if (g_in_block_loop)
		++g_last[3];
	ctx().sync();
}

struct WaveGroup {
	__device__ int lane0() const { return (int) threadIdx.x; }
	__device__ int lane1() const { return (int) threadIdx.x + 1; }
	__device__ int lanes() const { return CU_NB; }
	__device__ void sync() const { __syncthreads(); } // one wave: no s_barrier, only the wait for the LDS accesses
};

// status: 0, or smallest failing column + 1
template <bool LDLT, typename T>
__global__ __launch_bounds__(CU_NB) void diag_kernel(T *L, long lrs, long lcs, T *W, long wrs, long wcs, T *alpha, int j0, int nb, int rc, Coef<T> *tab, int *status)
{
	__shared__ DiagLocal<T, CU_NB, CU_RC> m;
	const int limit = LDLT ? nb : diag_limit(*status, j0, nb);
	if (limit == 0)
		return;
	const int done = diag_block<LDLT, CU_NB, CU_RC, T>(WaveGroup{}, m, L, lrs, lcs, W, wrs, wcs, alpha, nb, rc, limit, tab);
	if (!LDLT && done < limit && threadIdx.x == 0)
		*status = j0 + done + 1; // smaller than the word's value, if it had one
}

template <bool LDLT, int RCW, typename T>
__global__ __launch_bounds__(CU_TAIL_NT) void tail_kernel(T *L, long lrs, long lcs, T *W, long wrs, long wcs, long nrows, int nb, int rc, const Coef<T> *tab, const int *status)
{
	__shared__ Coef<T> ctab[CU_NB * RCW];
	if (!LDLT && *status != 0)
		return;
	for (int e = (int) threadIdx.x; e < nb * rc; e += CU_TAIL_NT)
		ctab[e] = tab[e];
	__syncthreads();
	const long i = (long) blockIdx.x * CU_TAIL_NT + threadIdx.x;
	if (i < nrows)
		tail_row<LDLT, RCW, T>(L + i * lrs, lcs, W + i * wrs, wcs, nb, rc, ctab);
}

template <bool LDLT, int RCW, typename T>
void launch_tail(MatV<T> Lt, MatV<T> Wt, int nb, int rc, const Coef<T> *tab, const int *status)
{
	const unsigned blocks = (unsigned) ((Lt.nrows + CU_TAIL_NT - 1) / CU_TAIL_NT);
	hipLaunchKernelGGL((tail_kernel<LDLT, RCW, T>), dim3(blocks), dim3(CU_TAIL_NT), 0, ctx().stream, Lt.p, Lt.rs, Lt.cs, Wt.p, Wt.rs, Wt.cs, Lt.nrows, nb, rc, tab,
			   status);
}

// L (n x n), W (n x r), alpha (r contiguous entries): device memory.  tab: CU_NB * r coefficients, status: one word (LLT).
template <bool LDLT, typename T> void rank_update_launches(MatV<T> L, MatV<T> W, T *alpha, Coef<T> *tab, int *status)
{
	const idx_t n = L.nrows, r = W.ncols;
	hipStream_t s = ctx().stream;
	g_last[2] = (long) ((r + CU_RC - 1) / CU_RC);
	g_in_block_loop = true;
	for (idx_t j0 = 0; j0 < n; j0 += CU_NB) {
		const int nb = (int) (n - j0 < CU_NB ? n - j0 : CU_NB);
		const idx_t below = n - j0 - nb;
		++g_last[0];
		for (idx_t k0 = 0; k0 < r; k0 += CU_RC) {
			const int rc = (int) (r - k0 < CU_RC ? r - k0 : CU_RC);
			Coef<T> *ct = tab + (size_t) k0 * CU_NB;
			const MatV<T> Ld = L.sub(j0, j0, nb, nb), Wd = W.sub(j0, k0, nb, rc);
			hipLaunchKernelGGL((diag_kernel<LDLT, T>), dim3(1), dim3(CU_NB), 0, s, Ld.p, Ld.rs, Ld.cs, Wd.p, Wd.rs, Wd.cs, alpha + k0, (int) j0, nb, rc, ct, status);
			if (below == 0 || g_diag_only.load(std::memory_order_relaxed))
				continue;
			const MatV<T> Lt = L.sub(j0 + nb, j0, below, nb), Wt = W.sub(j0 + nb, k0, below, rc);
			if (rc == 1)
				launch_tail<LDLT, 1, T>(Lt, Wt, nb, rc, ct, status);
			else if (rc <= 8)
				launch_tail<LDLT, 8, T>(Lt, Wt, nb, rc, ct, status);
			else
				launch_tail<LDLT, CU_RC, T>(Lt, Wt, nb, rc, ct, status);
			++g_last[1];
		}
	}
	g_in_block_loop = false;
	FH_HIP(hipGetLastError());
}

// the word of the call, read once after the last launch
long read_status(const int *status)
{
	int *h = ctx().pinned_ints();
	FH_HIP(hipMemcpyAsync(h, status, sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
	sync_stream();
	return h[0] == 0 ? -1 : (long) h[0] - 1;
}

size_t table_bytes(idx_t r, size_t elem) { return Arena::padded((size_t) CU_NB * (size_t) r * 3 * elem); }

// ---- deletion
// keep[q] = old index of row / column q of the compacted matrix, q < n - r
__global__ void keep_kernel(const long *idx, long r, long nkeep, long *keep)
{
	const long q = (long) blockIdx.x * blockDim.x + threadIdx.x;
	if (q < nkeep)
		keep[q] = kept_index(q, idx, r);
}

// W (m x r, column major, m = n - first - r) and alpha (r): update.rs:440-451, the entries the reference never reads zero filled
template <typename T> __global__ void delete_gather_kernel(const T *LD, long rs, long cs, const long *idx, const long *keep, long first, long m, long r, T *W, T *alpha)
{
	const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
	if (e < r)
		alpha[e] = LD[idx[e] * (rs + cs)];
	if (e >= m * r)
		return;
	const long t = e % m, k = e / m, i = keep[first + t], j = idx[k];
	W[e] = i > j ? LD[i * rs + j * cs] : (T) 0;
}

// C (n - first rows, column major, ld = n - first) <- rows [first, n) of the lower triangle of LD
template <typename T> __global__ void delete_copy_kernel(const T *LD, long rs, long cs, long first, long n, T *C)
{
	const long ld = n - first;
	const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= ld * n)
		return;
	const long t = e % ld, j = e / ld, i = first + t;
	if (j <= i)
		C[e] = LD[i * rs + j * cs];
}

// update.rs:343-374 out of the copy: LD[p, q] <- old LD[keep[p], keep[q]], first <= p < n - r, q <= p
template <typename T> __global__ void delete_compact_kernel(T *LD, long rs, long cs, const long *keep, long first, long n, long nkeep, const T *C)
{
	const long ld = n - first, rows = nkeep - first;
	const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= rows * nkeep)
		return;
	const long p = first + e % rows, q = e / rows;
	if (q <= p)
		LD[p * rs + q * cs] = C[(keep[p] - first) + keep[q] * ld];
}

unsigned blocks_of(idx_t total) { return (unsigned) ((total + 255) / 256); }

} // namespace

void chol_update_last(long out[4])
{
	for (int i = 0; i < 4; ++i)
		out[i] = g_last[i];
}

void chol_update_debug_diag_only(int on) { g_diag_only.store(on ? 1 : 0, std::memory_order_relaxed); }

void chol_update_shape(int elem_bytes, size_t out[2])
{
	(void) elem_bytes; // one shape for both precisions
	out[0] = CU_NB;
	out[1] = CU_RC;
}

// L (n x n), W (n x r), alpha (r x 1): host or device memory, each on its own.  Returns -1, or the failing column (LLT).
template <typename T> long chol_rank_update(MatV<T> L, MatV<T> W, MatV<T> alpha, bool ldlt)
{
	const idx_t n = L.nrows, r = W.ncols;
	g_last[0] = g_last[1] = g_last[2] = g_last[3] = 0;
	FH_CHECK(n < ((idx_t) 1 << 30) && r < ((idx_t) 1 << 30), "cholesky update: dimension too large");
	const bool l_host = !is_device_ptr(L.p), w_host = !is_device_ptr(W.p), a_host = !is_device_ptr(alpha.p);
	Arena ar(256 + Arena::padded((size_t) r * sizeof(T)) + table_bytes(r, sizeof(T)) + (l_host ? Arena::padded((size_t) n * n * sizeof(T)) : 0)
		 + (w_host ? Arena::padded((size_t) n * r * sizeof(T)) : 0) + 512);
	int *status = ar.take<int>(1);
	T *da;
	if (a_host) {
		da = ar.copy_in<T>(alpha.c()).p;
	} else {
		da = ar.take<T>((size_t) r);
		copy_dev<T>(MatV<T>{da, r, 1, 1, r}, alpha.c());
	}
	Coef<T> *tab = reinterpret_cast<Coef<T> *>(ar.take<T>((size_t) CU_NB * (size_t) r * 3));
	const MatV<T> dl = l_host ? ar.copy_in<T>(L.c()) : L, dw = w_host ? ar.copy_in<T>(W.c()) : W;
	long res = -1;
	if (ldlt) {
		rank_update_launches<true, T>(dl, dw, da, tab, status);
	} else {
		FH_HIP(hipMemsetAsync(status, 0, sizeof(int), ctx().stream));
		rank_update_launches<false, T>(dl, dw, da, tab, status);
		res = read_status(status);
	}
	if (l_host)
		Arena::copy_out<T>(L, dl.c());
	return res;
}

// LD (n x n, host or device), idx: r sorted distinct indices below n (host).  The leading (n - r)^2 block receives the factors.
template <typename T> void ldlt_delete_rows_and_cols(MatV<T> LD, const idx_t *idx, idx_t r)
{
	const idx_t n = LD.nrows, first = idx[0], nkeep = n - r, m = n - first - r;
	g_last[0] = g_last[1] = g_last[2] = g_last[3] = 0;
	FH_CHECK(n < ((idx_t) 1 << 30), "cholesky update: dimension too large");
	hipStream_t s = ctx().stream;
	const bool l_host = !is_device_ptr(LD.p);
	Arena ar(Arena::padded((size_t) r * sizeof(long)) + Arena::padded((size_t) (nkeep + 1) * sizeof(long)) + Arena::padded((size_t) r * sizeof(T))
		 + Arena::padded((size_t) (m * r + 1) * sizeof(T)) + Arena::padded((size_t) (n - first) * n * sizeof(T)) + table_bytes(r, sizeof(T))
		 + (l_host ? Arena::padded((size_t) n * n * sizeof(T)) : 0) + 512);
	long *didx = ar.take<long>((size_t) r), *keep = ar.take<long>((size_t) nkeep + 1);
	T *da = ar.take<T>((size_t) r), *dw = ar.take<T>((size_t) (m * r + 1)), *copy = ar.take<T>((size_t) (n - first) * (size_t) n);
	Coef<T> *tab = reinterpret_cast<Coef<T> *>(ar.take<T>((size_t) CU_NB * (size_t) r * 3));
	const MatV<T> dl = l_host ? ar.copy_in<T>(LD.c()) : LD;
	FH_HIP(hipMemcpyAsync(didx, idx, (size_t) r * sizeof(long), hipMemcpyHostToDevice, s));
	sync_stream(); // idx is the caller's memory
	if (nkeep > 0)
		hipLaunchKernelGGL(keep_kernel, dim3(blocks_of(nkeep)), dim3(256), 0, s, didx, (long) r, (long) nkeep, keep);
	const idx_t ge = m * r > r ? m * r : r;
	hipLaunchKernelGGL((delete_gather_kernel<T>), dim3(blocks_of(ge)), dim3(256), 0, s, dl.p, dl.rs, dl.cs, didx, keep, (long) first, (long) m, (long) r, dw, da);
	if (m > 0) {
		hipLaunchKernelGGL((delete_copy_kernel<T>), dim3(blocks_of((n - first) * n)), dim3(256), 0, s, dl.p, dl.rs, dl.cs, (long) first, (long) n, copy);
		hipLaunchKernelGGL((delete_compact_kernel<T>), dim3(blocks_of(m * nkeep)), dim3(256), 0, s, dl.p, dl.rs, dl.cs, keep, (long) first, (long) n, (long) nkeep,
				   copy);
		FH_HIP(hipGetLastError());
		rank_update_launches<true, T>(dl.sub(first, first, m, m), MatV<T>{dw, m, r, 1, m}, da, tab, nullptr);
	}
	FH_HIP(hipGetLastError());
	if (l_host)
		Arena::copy_out<T>(LD, dl.c());
}

template long chol_rank_update<double>(MatV<double>, MatV<double>, MatV<double>, bool);
template long chol_rank_update<float>(MatV<float>, MatV<float>, MatV<float>, bool);
template void ldlt_delete_rows_and_cols<double>(MatV<double>, const idx_t *, idx_t);
template void ldlt_delete_rows_and_cols<float>(MatV<float>, const idx_t *, idx_t);

} // namespace fh
