// Cholesky factorization with diagonal pivoting P A P^T = L L^T of a symmetric positive semidefinite matrix (include/faer_hip.h
// section 2h; faer/src/linalg/cholesky/llt_pivoting/{factor,solve,reconstruct,inverse}.rs; LAPACK's pstrf).  Only the lower triangle of
// A is read or written.
//
//  * piv_llt_init_kernel, one workgroup: the scan of the diagonal that opens the factorization (negative / NaN entry, first pivot,
//    tol = eps n max) and, after a trailing update, the scan that opens the next panel.  It clears the running sums and leaves its
//    result as the one candidate the first pivot kernel of the panel combines.
//  * Panel of PL_NB columns while more than PL_NB rows remain, lazily updated (factor.rs:88-170).  Column j takes two launches:
//    piv_llt_pivot_kernel (one workgroup) combines the candidates of the previous launch in a fixed order, decides (NaN, tol, pivot),
//    swaps inside the lower triangle and writes sqrt(pivot); piv_llt_col_kernel (one workgroup per 256 rows) forms the column of L
//    from the panel's earlier columns, scales it, advances the running sums s_i += l_ij^2 and emits one candidate a_ii - s_i per
//    workgroup.  Every launch returns at once when the done word is set: no host synchronisation inside a panel.  After the panel: one
//    read-back of the state words, the LU row-interchange kernel on the columns left of the panel and one TriangularLower MFMA product
//    A22 -= A21 A21^T (diagonal included), skipped after an early stop.
//  * piv_llt_leaf_kernel, one workgroup: the last <= PL_NB rows as a full symmetric image in LDS, unblocked and eagerly updated.
//  * Ties of every arg-max go to the lowest index (strict >, candidates combined in ascending row order), as in the reference.
#include "common.h"
#include "perm.h"
#include <limits>

using namespace fh;

namespace {

constexpr int PL_NB = 64;   // panel width, most rows of the leaf: its fp64 image of 64 x 65 entries takes 33 KB of LDS
constexpr int PL_LDP = 65;  // pitch of the leaf's LDS image (odd: rows and columns are both conflict free)
constexpr int PL_NT = 256;  // threads of the leaf and of a column workgroup
constexpr int PL_PT = 1024; // threads of the init and pivot workgroups
constexpr int PL_NOIDX = 0x7fffffff;

// device state of a factorization
enum { PS_DONE = 0, PS_STATUS, PS_RANK, PS_INDEX, PS_COUNT = 4 };

// arg-max candidate of a set of diagonal entries: the largest positive one (v == 0, i == PL_NOIDX: none) and "one of them is NaN"
// (the opening scan: "or negative")
template <typename T> struct PCand {
	T v;
	int i;
	int bad;
};

// larger value wins, equal values: the lower index
template <typename T> static __device__ __forceinline__ void cand_merge(PCand<T> &a, T ov, int oi, int ob)
{
	if (ov > a.v || (ov == a.v && oi < a.i)) {
		a.v = ov;
		a.i = oi;
	}
	a.bad |= ob;
}

template <typename T> static __device__ __forceinline__ void wave_cand(PCand<T> &a)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const T ov = __shfl_xor(a.v, off, 64);
		const int oi = __shfl_xor(a.i, off, 64);
		const int ob = __shfl_xor(a.bad, off, 64);
		cand_merge(a, ov, oi, ob);
	}
}

// workgroup reduction of NT threads; every thread returns with the result.  s: NT / 64 entries.
template <typename T, int NT> static __device__ __forceinline__ void block_cand(PCand<T> &a, PCand<T> *s)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	wave_cand(a);
	__syncthreads(); // s may still be read from the previous use
	if (lane == 0)
		s[wave] = a;
	__syncthreads();
	a = s[0];
#pragma unroll
	for (int w = 1; w < NT / 64; ++w)
		cand_merge(a, s[w].v, s[w].i, s[w].bad);
}

// one diagonal entry d of row r joins the candidate
template <typename T> static __device__ __forceinline__ void cand_take(PCand<T> &a, T d, int r)
{
	if (d != d) {
		a.bad = 1;
	} else if (d > a.v) {
		a.v = d;
		a.i = r;
	}
}

// Scan of the diagonal from row k on (factor.rs:76-86 with first != 0, :94-97 and :105-119 at the start of a later panel); clears the
// running sums of those rows.  first: a negative entry counts as bad, the state words and tol are initialised.
template <typename T>
__global__ __launch_bounds__(PL_PT) void piv_llt_init_kernel(const T *A, idx_t rs, idx_t cs, int n, int k, T *sums, int *st, T *fv,
							     PCand<T> *cands, int first)
{
	__shared__ PCand<T> s_c[PL_PT / 64];
	if (!first && st[PS_DONE])
		return;
	const int tid = threadIdx.x;
	PCand<T> c{(T) 0, PL_NOIDX, 0};
	for (int r = k + tid; r < n; r += PL_PT) { // (ascending rows: the first maximum)
		const T x = A[(idx_t) r * (rs + cs)];
		sums[r] = (T) 0;
		if (first && x < (T) 0)
			c.bad = 1;
		cand_take(c, x, r);
	}
	block_cand<T, PL_PT>(c, s_c);
	if (tid == 0) {
		cands[0] = c;
		if (first) { // a bad diagonal of A is decided here: a matrix of <= PL_NB rows goes to the leaf without a pivot kernel
			st[PS_DONE] = c.bad;
			st[PS_STATUS] = c.bad;
			st[PS_RANK] = n;
			st[PS_INDEX] = 0;
			fv[0] = std::numeric_limits<T>::epsilon() * (T) n * c.v;
		}
	}
}

// One workgroup: the decision of step j of the panel that starts at column k and the symmetric swap j <-> pvt inside the lower
// triangle (factor.rs:105-156).  piv_rel / piv_abs: the pivot row relative to k (for the row-interchange kernel) and absolute.
template <typename T>
__global__ __launch_bounds__(PL_PT) void piv_llt_pivot_kernel(T *A, idx_t rs, idx_t cs, int n, int k, int j, T *sums, int *st, const T *fv,
							      const PCand<T> *cands, int ncand, int *piv_rel, int *piv_abs)
{
	__shared__ PCand<T> s_c[PL_PT / 64];
	if (st[PS_DONE])
		return;
	const int tid = threadIdx.x;
	PCand<T> c{(T) 0, PL_NOIDX, 0};
	for (int w = tid; w < ncand; w += PL_PT) // (ascending w: ascending rows)
		cand_merge(c, cands[w].v, cands[w].i, cands[w].bad);
	block_cand<T, PL_PT>(c, s_c);
	if (c.bad) {
		if (tid == 0) {
			st[PS_STATUS] = 1;
			st[PS_INDEX] = j;
			st[PS_DONE] = 1;
		}
		return;
	}
	const int pvt = c.i == PL_NOIDX ? j : c.i;
	const T ajj = c.v;
	if (j > 0 && ajj < fv[0]) {
		if (tid == 0) {
			st[PS_RANK] = j;
			A[(idx_t) j * (rs + cs)] = ajj;
			st[PS_DONE] = 1;
		}
		return;
	}
	if (pvt != j) {
		for (int cc = k + tid; cc < j; cc += PL_PT) { // rows j, pvt of the panel's earlier columns
			T *p = A + (idx_t) cc * cs;
			const T x = p[(idx_t) j * rs];
			p[(idx_t) j * rs] = p[(idx_t) pvt * rs];
			p[(idx_t) pvt * rs] = x;
		}
		for (int r = pvt + 1 + tid; r < n; r += PL_PT) { // columns j, pvt below row pvt
			T *p = A + (idx_t) r * rs;
			const T x = p[(idx_t) j * cs];
			p[(idx_t) j * cs] = p[(idx_t) pvt * cs];
			p[(idx_t) pvt * cs] = x;
		}
		for (int t = j + 1 + tid; t < pvt; t += PL_PT) { // column j between the rows <-> row pvt between the columns
			T *p = A + (idx_t) t * rs + (idx_t) j * cs, *q = A + (idx_t) pvt * rs + (idx_t) t * cs;
			const T x = *p;
			*p = *q;
			*q = x;
		}
		if (tid == 0) {
			A[(idx_t) pvt * (rs + cs)] = A[(idx_t) j * (rs + cs)];
			const T x = sums[j];
			sums[j] = sums[pvt];
			sums[pvt] = x;
		}
	}
	if (tid == 0) {
		piv_rel[j] = pvt - k;
		piv_abs[j] = pvt;
		A[(idx_t) j * (rs + cs)] = sqrt(ajj);
	}
}

// Column j of L below the diagonal, one row per thread (factor.rs:157-169), fused with the next step's candidate diagonal
// (factor.rs:99-103): a(i, j) = (a(i, j) - sum_{c = k}^{j - 1} a(i, c) a(j, c)) / a(j, j), s_i += a(i, j)^2, candidate a(i, i) - s_i.
template <typename T>
__global__ __launch_bounds__(PL_NT) void piv_llt_col_kernel(T *A, idx_t rs, idx_t cs, int n, int k, int j, T *sums, const int *st,
							    PCand<T> *cands)
{
	__shared__ PCand<T> s_c[PL_NT / 64];
	__shared__ T s_row[PL_NB];
	if (st[PS_DONE])
		return;
	const int tid = threadIdx.x;
	const int w = j - k; // < PL_NB
	if (tid < w)
		s_row[tid] = A[(idx_t) j * rs + (idx_t) (k + tid) * cs];
	__syncthreads();
	const T dinv = (T) 1 / A[(idx_t) j * (rs + cs)];
	const int r = j + 1 + blockIdx.x * PL_NT + tid;
	PCand<T> c{(T) 0, PL_NOIDX, 0};
	if (r < n) {
		T *ar = A + (idx_t) r * rs;
		T acc = ar[(idx_t) j * cs];
		for (int cc = 0; cc < w; ++cc)
			acc = fh_fma(-ar[(idx_t) (k + cc) * cs], s_row[cc], acc);
		const T l = acc * dinv;
		ar[(idx_t) j * cs] = l;
		const T s = sums[r] + l * l;
		sums[r] = s;
		cand_take(c, A[(idx_t) r * (rs + cs)] - s, r);
	}
	block_cand<T, PL_NT>(c, s_c);
	if (tid == 0)
		cands[blockIdx.x] = c;
}

// ------------------------------------------------------------------------------------------------ leaf
// The trailing m x m block (m <= PL_NB) that starts at row / column k0, unblocked and eagerly updated on a symmetric image in LDS.
// Every wavefront takes the pivot decision redundantly from the same image.
template <typename T>
__global__ __launch_bounds__(PL_NT) void piv_llt_leaf_kernel(T *A, idx_t rs, idx_t cs, int n, int k0, int *st, const T *fv, int *piv_rel,
							     int *piv_abs)
{
	__shared__ T S[PL_NB * PL_LDP];
	__shared__ int s_piv[PL_NB];
	if (st[PS_DONE])
		return;
	const int tid = threadIdx.x, lane = tid & 63;
	const int m = n - k0;
	T *Ab = A + (idx_t) k0 * (rs + cs);
	const T tol = fv[0];
	for (int e = tid; e < m * m; e += PL_NT) {
		const int i = e % m, j = e / m;
		S[j * PL_LDP + i] = j <= i ? Ab[(idx_t) i * rs + (idx_t) j * cs] : Ab[(idx_t) j * rs + (idx_t) i * cs];
	}
	int done_at = m; // columns of L the leaf completed
	for (int j = 0; j < m; ++j) {
		__syncthreads();
		PCand<T> c{(T) 0, PL_NOIDX, 0};
		if (lane >= j && lane < m)
			cand_take(c, S[lane * PL_LDP + lane], lane);
		wave_cand(c);
		if (c.bad) {
			if (tid == 0) {
				st[PS_STATUS] = 1;
				st[PS_INDEX] = k0 + j;
				st[PS_DONE] = 1;
			}
			return;
		}
		const int pvt = c.i == PL_NOIDX ? j : c.i;
		const T ajj = c.v;
		if (k0 + j > 0 && ajj < tol) {
			__syncthreads();
			if (tid == 0)
				S[j * PL_LDP + j] = ajj;
			done_at = j;
			break;
		}
		__syncthreads();
		if (pvt != j) { // P S P^T: rows, then columns
			if (tid < m) {
				const T x = S[tid * PL_LDP + j];
				S[tid * PL_LDP + j] = S[tid * PL_LDP + pvt];
				S[tid * PL_LDP + pvt] = x;
			}
			__syncthreads();
			if (tid < m) {
				const T x = S[j * PL_LDP + tid];
				S[j * PL_LDP + tid] = S[pvt * PL_LDP + tid];
				S[pvt * PL_LDP + tid] = x;
			}
			__syncthreads();
		}
		const T root = sqrt(ajj);
		const T dinv = (T) 1 / root;
		const int mm = m - j - 1;
		for (int e = tid; e < mm * mm; e += PL_NT) {
			const int i = j + 1 + e % mm, cc = j + 1 + e / mm;
			if (i < cc)
				continue;
			const T li = S[j * PL_LDP + i] * dinv, lc = S[j * PL_LDP + cc] * dinv;
			const T v = fh_fma(-li, lc, S[cc * PL_LDP + i]);
			S[cc * PL_LDP + i] = v;
			S[i * PL_LDP + cc] = v;
		}
		__syncthreads();
		if (tid > j && tid < m)
			S[j * PL_LDP + tid] *= dinv;
		if (tid == 0) {
			S[j * PL_LDP + j] = root;
			s_piv[j] = pvt;
		}
	}
	__syncthreads();
	for (int e = tid; e < m * m; e += PL_NT) {
		const int i = e % m, j = e / m;
		if (j <= i)
			Ab[(idx_t) i * rs + (idx_t) j * cs] = S[j * PL_LDP + i];
	}
	if (tid < done_at) {
		piv_rel[k0 + tid] = s_piv[tid];
		piv_abs[k0 + tid] = k0 + s_piv[tid];
	}
	if (tid == 0 && done_at < m) {
		st[PS_RANK] = k0 + done_at;
		st[PS_DONE] = 1;
	}
}

thread_local size_t g_last[4] = {0, 0, 0, 0}; // panels, leaf rows, columns factored, host synchronisations inside panels

struct PivLltResult {
	int status = 0; // 0 Ok, 1 NonPositivePivot
	idx_t rank = 0, index = 0;
	long count = 0;
};

// the state words (one host synchronisation)
void read_state(const int *st, int *out)
{
	int *h = ctx().pinned_ints();
	FH_HIP(hipMemcpyAsync(h, st, (size_t) PS_COUNT * sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
	ctx().sync();
	for (int i = 0; i < PS_COUNT; ++i)
		out[i] = h[i];
}

// A: n x n device view.  perm / perm_inv: host, n entries.
template <typename T> PivLltResult piv_llt_dev(MatV<T> A, idx_t *perm, idx_t *perm_inv)
{
	const idx_t n = A.nrows;
	PivLltResult res;
	g_last[0] = g_last[1] = g_last[2] = g_last[3] = 0;
	if (n == 0)
		return res;
	FH_CHECK(n < ((idx_t) 1 << 30), "piv_llt: dimension too large");
	hipStream_t s = ctx().stream;
	const int ni = (int) n;
	const int nwg_max = (ni + PL_NT - 1) / PL_NT;
	Scratch stb(64), fvb(64), pivb((size_t) 2 * n * sizeof(int)), sumb((size_t) n * sizeof(T)), cab((size_t) nwg_max * sizeof(PCand<T>));
	int *st = stb.as<int>(), *piv_rel = pivb.as<int>(), *piv_abs = pivb.as<int>() + n;
	T *fv = fvb.as<T>(), *sums = sumb.as<T>();
	PCand<T> *cands = cab.as<PCand<T>>();
	hipLaunchKernelGGL(piv_llt_init_kernel<T>, dim3(1), dim3(PL_PT), 0, s, A.p, A.rs, A.cs, ni, 0, sums, st, fv, cands, 1);
	int h[PS_COUNT] = {0, 0, ni, 0};
	int k0 = 0;
	while (ni - k0 > PL_NB) {
		if (k0 > 0)
			hipLaunchKernelGGL(piv_llt_init_kernel<T>, dim3(1), dim3(PL_PT), 0, s, A.p, A.rs, A.cs, ni, k0, sums, st, fv, cands, 0);
		int ncand = 1;
		for (int j = k0; j < k0 + PL_NB; ++j) {
			hipLaunchKernelGGL(piv_llt_pivot_kernel<T>, dim3(1), dim3(PL_PT), 0, s, A.p, A.rs, A.cs, ni, k0, j, sums, st, fv, cands, ncand,
					   piv_rel, piv_abs);
			ncand = (ni - j - 1 + PL_NT - 1) / PL_NT; // >= 1: more than PL_NB rows remain at k0
			hipLaunchKernelGGL(piv_llt_col_kernel<T>, dim3(ncand), dim3(PL_NT), 0, s, A.p, A.rs, A.cs, ni, k0, j, sums, st, cands);
		}
		FH_HIP(hipGetLastError());
		read_state(st, h);
		++g_last[0];
		if (h[PS_STATUS] != 0)
			break;
		const int cols = h[PS_DONE] ? h[PS_RANK] - k0 : PL_NB;
		FH_CHECK(cols >= 0 && cols <= PL_NB, "piv_llt: panel ended at an unexpected column");
		if (k0 > 0 && cols > 0)
			laswp_rows_dev<T>(A.sub(k0, 0, n - k0, k0), piv_rel + k0, cols); // factor.rs:129-133 on the columns left of the panel
		if (h[PS_DONE])
			break;
		const idx_t k1 = k0 + PL_NB, mr = n - k1;
		// factor.rs:171-181
		matmul_triangular_dev<T>(A.sub(k1, k1, mr, mr), (int) FaerBlock_TriangularLower, true, A.sub(k1, k0, mr, PL_NB).c(),
					 (int) FaerBlock_Rectangular, A.sub(k1, k0, mr, PL_NB).t().c(), (int) FaerBlock_Rectangular, (T) -1);
		k0 = (int) k1;
	}
	if (!h[PS_DONE]) {
		const int m = ni - k0;
		hipLaunchKernelGGL(piv_llt_leaf_kernel<T>, dim3(1), dim3(PL_NT), 0, s, A.p, A.rs, A.cs, ni, k0, st, fv, piv_rel, piv_abs);
		FH_HIP(hipGetLastError());
		read_state(st, h);
		g_last[1] = (size_t) m;
		const int cols = h[PS_STATUS] != 0 ? 0 : (h[PS_DONE] ? h[PS_RANK] - k0 : m);
		FH_CHECK(cols >= 0 && cols <= m, "piv_llt: leaf ended at an unexpected column");
		if (k0 > 0 && cols > 0)
			laswp_rows_dev<T>(A.sub(k0, 0, m, k0), piv_rel + k0, cols);
	}
	if (h[PS_STATUS] != 0) {
		ctx().sync();
		res.status = 1;
		res.index = h[PS_INDEX];
		return res;
	}
	res.rank = h[PS_RANK];
	FH_CHECK(res.rank >= 0 && res.rank <= n, "piv_llt: rank out of range");
	std::vector<int> hp((size_t) res.rank);
	if (res.rank > 0)
		FH_HIP(hipMemcpyAsync(hp.data(), piv_abs, (size_t) res.rank * sizeof(int), hipMemcpyDeviceToHost, s));
	ctx().sync();
	g_last[2] = (size_t) res.rank;
	// factor.rs:63-65, :127, :153, :187-189
	res.count = perm_from_transpositions("piv_llt", n, res.rank, [&](idx_t j) { return (idx_t) hp[(size_t) j]; }, perm, perm_inv);
	return res;
}

template <typename T, typename I> FaerPivLltStatus factor_api(FaerMatMut A, FaerSliceMut pf, FaerSliceMut pb)
{
	const idx_t n = (idx_t) A.nrows;
	FH_CHECK(A.nrows == A.ncols, "piv_llt: matrix must be square");
	std::vector<idx_t> perm((size_t) n), perm_inv((size_t) n);
	PivLltResult r;
	{
		Staged<T> a(view<T>(A), true, true);
		r = piv_llt_dev<T>(a.dev, perm.data(), perm_inv.data());
	}
	FaerPivLltStatus stt;
	memset(&stt, 0, sizeof(stt));
	if (r.status != 0) {
		stt.tag = FaerPivLltStatus_NonPositivePivot;
		stt.non_positive_pivot.index = (size_t) r.index;
		return stt;
	}
	store_perm<I>("piv_llt", pf, pb, perm.data(), perm_inv.data(), n);
	stt.tag = FaerPivLltStatus_Ok;
	stt.ok.rank = (size_t) r.rank;
	stt.ok.transposition_count = (size_t) r.count;
	return stt;
}

// solve.rs:13-41
template <typename T, typename I> void solve_api(FaerMatRef L, FaerSliceRef pf, FaerSliceRef pb, FaerMatMut rhs)
{
	const size_t n = L.nrows;
	FH_CHECK(L.ncols == n && rhs.nrows == n, "piv_llt solve: dimension mismatch");
	FH_CHECK(rhs.ncols < 65536, "piv_llt solve: too many right-hand sides");
	DevPerm fwd("piv_llt solve", pf, (idx_t) n, I{}), bwd("piv_llt solve", pb, (idx_t) n, I{});
	if (n == 0 || rhs.ncols == 0)
		return;
	Staged<const T> l(view<T>(L), true, false);
	Staged<T> x(view<T>(rhs), true, true);
	permute_rows<T>(x.dev, fwd);
	trsm_lower_dev<T>(l.dev, false, x.dev);
	trsm_upper_dev<T>(l.dev.t(), false, x.dev);
	permute_rows<T>(x.dev, bwd);
}

// reconstruct.rs:12-52 / inverse.rs:12-54 (the lower triangle of out only)
template <typename T, typename I> void rebuild_api(FaerMatMut Out, FaerMatRef L, FaerSliceRef pf, FaerSliceRef pb, bool inverse)
{
	const idx_t n = (idx_t) L.nrows;
	FH_CHECK((idx_t) L.ncols == n && (idx_t) Out.nrows == n && (idx_t) Out.ncols == n, "piv_llt reconstruct / inverse: dimension mismatch");
	FH_CHECK(n < 65536, "piv_llt reconstruct / inverse: dimension too large");
	check_perm_slice("piv_llt reconstruct / inverse", pf, n);
	DevPerm bwd("piv_llt reconstruct / inverse", pb, n, I{});
	if (n == 0)
		return;
	Staged<const T> l(view<T>(L), true, false);
	Staged<T> o(view<T>(Out), true, true); // the strict upper triangle is kept
	Scratch tb((size_t) n * (size_t) n * sizeof(T) + 256);
	MatV<T> tmp{tb.as<T>(), n, n, 1, n};
	if (!inverse) {
		matmul_triangular_dev<T>(tmp, (int) FaerBlock_TriangularLower, false, l.dev, (int) FaerBlock_TriangularLower, l.dev.t(),
					 (int) FaerBlock_TriangularUpper, (T) 1);
	} else {
		Scratch wb((size_t) n * (size_t) n * sizeof(T) + 256);
		MatV<T> W{wb.as<T>(), n, n, 1, n};
		tri_invert_lower_dev<T>(W, l.dev, false);
		matmul_triangular_dev<T>(tmp, (int) FaerBlock_TriangularLower, false, W.t().c(), (int) FaerBlock_TriangularUpper, W.c(),
					 (int) FaerBlock_TriangularLower, (T) 1);
	}
	sym_gather<T>(o.dev, tmp.p, bwd); // reconstruct.rs:40-51, inverse.rs:42-53
	ctx().sync();
}

} // namespace

extern "C" {

void faer_hip_debug_piv_llt_last(size_t out[4])
{
	for (int i = 0; i < 4; ++i)
		out[i] = g_last[i];
}

#define X(suf, T)                                                                                                                                  \
	FaerPivLltParams libfaer_v0_23_PivLltParams_##suf(void) { return FaerPivLltParams{128}; }
X(f64, double)
X(f32, float)
#undef X

#define X(it, I, suf, T)                                                                                                                           \
	FaerLayout libfaer_v0_23_piv_llt_factor_in_place_scratch_##it##_##suf(size_t dim, FaerPar par, FaerPivLltParams params)                    \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) params;                                                                                                                     \
		return layout(2 * dim * sizeof(T), 64); /* factor.rs:37-45 */                                                                         \
	}                                                                                                                                          \
	FaerPivLltStatus libfaer_v0_23_piv_llt_factor_in_place_##it##_##suf(FaerMatMut A, FaerSliceMut perm_fwd, FaerSliceMut perm_bwd,            \
									    FaerPar par, FaerMemAlloc mem, FaerPivLltParams params)                \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		(void) params;                                                                                                                     \
		return factor_api<T, I>(A, perm_fwd, perm_bwd);                                                                                    \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_piv_llt_solve_in_place_scratch_##it##_##suf(size_t dim, size_t rhs_ncols, FaerPar par)                            \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * rhs_ncols * sizeof(T), 64); /* solve.rs:4-11 */                                                                   \
	}                                                                                                                                          \
	void libfaer_v0_23_piv_llt_solve_in_place_##it##_##suf(FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerConj A_conj,        \
							       FaerMatMut rhs, FaerPar par, FaerMemAlloc mem)                                      \
	{                                                                                                                                          \
		(void) A_conj;                                                                                                                     \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		solve_api<T, I>(L, perm_fwd, perm_bwd, rhs);                                                                                       \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_piv_llt_reconstruct_scratch_##it##_##suf(size_t dim, FaerPar par)                                                 \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * dim * sizeof(T), 64); /* reconstruct.rs:4-10 */                                                                   \
	}                                                                                                                                          \
	void libfaer_v0_23_piv_llt_reconstruct_##it##_##suf(FaerMatMut A, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, \
							    FaerMemAlloc mem)                                                                      \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		rebuild_api<T, I>(A, L, perm_fwd, perm_bwd, false);                                                                                \
	}                                                                                                                                          \
	FaerLayout libfaer_v0_23_piv_llt_inverse_scratch_##it##_##suf(size_t dim, FaerPar par)                                                     \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		return layout(dim * dim * sizeof(T), 64); /* inverse.rs:4-10 */                                                                       \
	}                                                                                                                                          \
	void libfaer_v0_23_piv_llt_inverse_##it##_##suf(FaerMatMut A_inv, FaerMatRef L, FaerSliceRef perm_fwd, FaerSliceRef perm_bwd, FaerPar par, \
							FaerMemAlloc mem)                                                                          \
	{                                                                                                                                          \
		(void) par;                                                                                                                        \
		(void) mem;                                                                                                                        \
		rebuild_api<T, I>(A_inv, L, perm_fwd, perm_bwd, true);                                                                             \
	}
X(u32, uint32_t, f64, double)
X(u64, uint64_t, f64, double)
X(u32, uint32_t, f32, float)
X(u64, uint64_t, f32, float)
#undef X

} // extern "C"
