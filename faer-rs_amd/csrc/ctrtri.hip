// Complex triangular inverse for c32 / c64: tri_invert_lower_dev<Cx<R>>.
//
// Driver: the recursion of the real path (extras.hip; faer/src/linalg/triangular_inverse.rs:43-123).  The E x E diagonal blocks are
// inverted by the leaf below, all of them in one launch, straight into the lower triangle of dst; every level above is two structured
// complex products per pair of h-wide diagonal blocks (cgemm.hip): T = src_bl * dst_tl, dst_bl = -dst_br * T.  Only the lower triangle
// of src is read and only the lower triangle of dst written (unit: neither diagonal is touched).
//
// Leaf (the new kernel of this file): one 256-thread workgroup per diagonal block, the block resident in LDS as re / im planes.
//   1. the reciprocals of the diagonal, once per entry; the SB x SB diagonal sub-blocks by substitution, one thread per column
//      (ctrtri_core.h), plain FMAs;
//   2. doubling, s = SB, 2 SB, ..., E / 2: W10 = -W11 (T10 W00) on the MFMA pipe, four real MFMAs per complex one as in cgemm.hip,
//      one 16 x 16 tile of the result per wavefront.
// LDS layout: the plane keeps the finished part of the inverse TWICE, W(i, j) at (i, j) and mirrored at (j, i), so that both the left
// operand (W11, walked down its columns) and the right operand (W00, walked along its rows) are read with the lanes of a fragment on
// consecutive addresses.  With the leading dimension LD = 16 mod 32 the two k-slices of a 32-lane group then sit in opposite halves of
// the 32 element-wide bank window: no bank conflict for ds_read_b32 (c32) or ds_read_b64 (c64).  A diagonal 16 x 16 tile holds both
// triangles of itself; the half that is zero in the operand is masked in registers.  The intermediate T10 W00 goes through a second,
// row-major pair of planes (leading dimension LDP = 16 mod 32) and is read back the same way.
// No barrier sits inside divergent control flow: the tile loops are wave uniform, the barriers are between them.
#include <algorithm>

#include "arena.h"
#include "common.h"
#include "ctrtri_core.h"
#include "mfma.h"

namespace fh {

namespace {

using namespace ctrtri;

constexpr int NT = 256;	      // threads of the leaf
constexpr int LD = E + 16;    // leading dimension of the block planes (16 mod 32)
constexpr int PH = E / 2;     // edge of the largest intermediate product
constexpr int LDP = PH + 16;  // its leading dimension (row major; 16 mod 32)
static_assert(LD % 32 == 16 && LDP % 32 == 16 && E % (2 * SB) == 0 && SB == 16 && E <= NT, "leaf layout");

template <typename R> constexpr size_t leaf_lds() { return (size_t) 2 * (E * LD + PH * LDP) * sizeof(R); }
static_assert(leaf_lds<double>() <= 112 * 1024, "LDS of a c64 leaf");

template <typename R> static __device__ __forceinline__ Cx<R> ct_ld(const Cx<R> *p, int vec)
{
	typedef R v2 __attribute__((ext_vector_type(2)));
	if (vec) {
		const v2 t = *reinterpret_cast<const v2 *>(p);
		return Cx<R>{t.x, t.y};
	}
	return Cx<R>{p->re, p->im};
}
template <typename R> static __device__ __forceinline__ void ct_st(Cx<R> *p, R re, R im, int vec)
{
	typedef R v2 __attribute__((ext_vector_type(2)));
	if (vec) {
		v2 t;
		t.x = re;
		t.y = im;
		*reinterpret_cast<v2 *>(p) = t;
	} else {
		p->re = re;
		p->im = im;
	}
}

// block b of the launch: rows / columns [b * E, b * E + nb) of src -> the same part of dst
template <typename R>
__global__ __launch_bounds__(NT) void ctrtri_leaf_kernel(const Cx<R> *__restrict__ src, idx_t srs, idx_t scs, Cx<R> *dst, idx_t drs, idx_t dcs, int n,
							 int unit, int svec, int dvec, int s_row_major, int d_row_major)
{
	typedef typename Mfma<R>::acc_t acc_t;
	extern __shared__ __align__(16) unsigned char ctrtri_smem[];
	R *pre = reinterpret_cast<R *>(ctrtri_smem);
	R *pim = pre + E * LD;
	R *qre = pim + E * LD;
	R *qim = qre + PH * LDP;
	__shared__ R s_ivr[E], s_ivi[E];

	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int l15 = lane & 15, lhi = lane >> 4;
	const int r0 = blockIdx.x * E;
	const int nb = min(E, n - r0);
	src += (idx_t) r0 * srs + (idx_t) r0 * scs;
	dst += (idx_t) r0 * drs + (idx_t) r0 * dcs;

	// the lower triangle (unit: strictly lower, ones on the diagonal), identity past nb, zeros above: nothing else of src is read
	for (int e = tid; e < E * E; e += NT) {
		const int i = s_row_major ? e / E : e % E, j = s_row_major ? e % E : e / E;
		Cx<R> v{(R) (i == j ? 1 : 0), (R) 0};
		if (i < nb && j < nb && (i > j || (i == j && !unit)))
			v = ct_ld(src + (idx_t) i * srs + (idx_t) j * scs, svec);
		pre[j * LD + i] = v.re;
		pim[j * LD + i] = v.im;
	}
	__syncthreads();

	// ---- 1. reciprocals, then the diagonal sub-blocks by substitution: thread (sub-block tid / SB, column tid % SB)
	if (tid < E) {
		R ir = (R) 1, ii = (R) 0;
		if (!unit)
			ct_recip(pre[tid * LD + tid], pim[tid * LD + tid], ir, ii);
		s_ivr[tid] = ir;
		s_ivi[tid] = ii;
	}
	__syncthreads();
	R wr[SB], wi[SB];
	const int c0 = (tid / SB) * SB, wj = tid % SB;
	if (tid < E)
		ct_column(pre + c0 * LD + c0, pim + c0 * LD + c0, LD, s_ivr + c0, s_ivi + c0, wj, wr, wi);
	__syncthreads(); // every column is computed from T before any of them replaces it
	if (tid < E) {
#pragma unroll
		for (int i = 0; i < SB; ++i)
			if (i >= wj) {
				pre[(c0 + wj) * LD + c0 + i] = wr[i];
				pim[(c0 + wj) * LD + c0 + i] = wi[i];
				pre[(c0 + i) * LD + c0 + wj] = wr[i]; // the mirror
				pim[(c0 + i) * LD + c0 + wj] = wi[i];
			}
	}
	__syncthreads();

	// ---- 2. doubling
#pragma unroll
	for (int s = SB; s < E; s *= 2) {
		const int ts = s / 16;		       // tiles along the edge of a block
		const int ntiles = (E / (2 * s)) * ts * ts; // over all pairs: 2 (s = 16), 4 (s = 32)
		// P = T10 W00: tile (ti, tj) sums over the tiles kt >= tj of the lower-triangular W00
		for (int t = wave; t < ntiles; t += NT / 64) {
			const int p = t / (ts * ts), ti = (t / ts) % ts, tj = t % ts;
			const int c = p * 2 * s;
			acc_t cre = (acc_t) (R) 0, cim = (acc_t) (R) 0;
			const int j = tj * 16 + l15;
			for (int k0 = tj * 16; k0 < s; k0 += 4) {
				const int k = k0 + lhi;
				const int oa = (c + k) * LD + c + s + ti * 16 + l15; // T10(i, k)
				const int ob = (c + k) * LD + c + j;		       // W00(k, j), from the mirror (j, k)
				const R ar = pre[oa], ai = pim[oa];
				const bool in = k >= j;
				const R br = in ? pre[ob] : (R) 0, bi = in ? pim[ob] : (R) 0;
				cre = Mfma<R>::run(ar, br, cre);
				cim = Mfma<R>::run(ar, bi, cim);
				cre = Mfma<R>::run(ai, -bi, cre);
				cim = Mfma<R>::run(ai, br, cim);
			}
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int o = (ti * 16 + Mfma<R>::row(r, lhi)) * LDP + p * s + j;
				qre[o] = cre[r];
				qim[o] = cim[r];
			}
		}
		__syncthreads();
		// W10 = -W11 P: tile (ti, tj) sums over the tiles kt <= ti of the lower-triangular W11
		for (int t = wave; t < ntiles; t += NT / 64) {
			const int p = t / (ts * ts), ti = (t / ts) % ts, tj = t % ts;
			const int c = p * 2 * s;
			acc_t cre = (acc_t) (R) 0, cim = (acc_t) (R) 0;
			const int i = ti * 16 + l15;
			for (int k0 = 0; k0 < (ti + 1) * 16; k0 += 4) {
				const int k = k0 + lhi;
				const int oa = (c + s + k) * LD + c + s + i; // W11(i, k)
				const int ob = k * LDP + p * s + tj * 16 + l15; // P(k, j)
				const bool in = i >= k;
				const R ar = in ? pre[oa] : (R) 0, ai = in ? pim[oa] : (R) 0;
				const R br = qre[ob], bi = qim[ob];
				cre = Mfma<R>::run(ar, br, cre);
				cim = Mfma<R>::run(ar, bi, cim);
				cre = Mfma<R>::run(ai, -bi, cre);
				cim = Mfma<R>::run(ai, br, cim);
			}
			// over T10, which the first product has consumed, and into the mirror (rows of the pair's first block: not an operand here)
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int row = c + s + ti * 16 + Mfma<R>::row(r, lhi), col = c + tj * 16 + l15;
				pre[col * LD + row] = -cre[r];
				pim[col * LD + row] = -cim[r];
				pre[row * LD + col] = -cre[r];
				pim[row * LD + col] = -cim[r];
			}
		}
		__syncthreads();
	}

	for (int e = tid; e < E * E; e += NT) {
		const int i = d_row_major ? e / E : e % E, j = d_row_major ? e % E : e / E;
		if (i < nb && j < nb && (unit ? i > j : i >= j))
			ct_st(dst + (idx_t) i * drs + (idx_t) j * dcs, pre[j * LD + i], pim[j * LD + i], dvec);
	}
}

inline idx_t iabs_(idx_t x) { return x < 0 ? -x : x; }

// the product buffer of the levels: hmax x hmax, hmax the widest diagonal block that still has a partner
inline idx_t level_hmax(idx_t n)
{
	idx_t hmax = E;
	while (hmax * 2 < n)
		hmax *= 2;
	return hmax;
}

template <typename R> void ctrtri_run(MatV<Cx<R>> dst, MatV<const Cx<R>> src, bool unit)
{
	typedef Cx<R> T;
	const idx_t n = src.nrows;
	FH_CHECK(src.ncols == n && dst.nrows == n && dst.ncols == n, "triangular inverse: dimension mismatch");
	if (n == 0)
		return;
	FH_CHECK(n < (1L << 30), "triangular inverse: matrix too large");
	ctx().ensure_device();
	const idx_t nblk = (n + E - 1) / E;
	raise_dynamic_lds<ctrtri_leaf_kernel<R>>(leaf_lds<R>());
	hipLaunchKernelGGL(ctrtri_leaf_kernel<R>, dim3((unsigned) nblk), dim3(NT), leaf_lds<R>(), ctx().stream, src.p, src.rs, src.cs, dst.p, dst.rs, dst.cs,
			   (int) n, unit ? 1 : 0, (int) (reinterpret_cast<uintptr_t>(src.p) % sizeof(T) == 0), (int) (reinterpret_cast<uintptr_t>(dst.p) % sizeof(T) == 0),
			   (int) (iabs_(src.cs) < iabs_(src.rs)), (int) (iabs_(dst.cs) < iabs_(dst.rs)));
	FH_HIP(hipGetLastError());
	if (nblk == 1)
		return;
	// levels: pairs of h-wide diagonal blocks (h = E, 2 E, ...): dst_bl = -dst_br * (src_bl * dst_tl)
	const int tri = unit ? 5 /* unit lower */ : 1 /* lower */;
	const idx_t hmax = level_hmax(n);
	Arena arena(Arena::padded((size_t) hmax * (size_t) hmax * sizeof(T)));
	T *tb = arena.take<T>((size_t) hmax * (size_t) hmax);
	for (idx_t h = E; h < n; h *= 2)
		for (idx_t base = 0; base + h < n; base += 2 * h) {
			const idx_t h2 = std::min(n - base - h, h); // ragged last pair
			MatV<T> Tm{tb, h2, h, 1, h2};
			// T = src_bl * dst_tl        (triangular_inverse.rs:64-74; rhs structured: only its lower triangle is read)
			matmul_triangular_dev<T>(Tm, 0, false, src.sub(base + h, base, h2, h), 0, dst.sub(base, base, h, h).c(), tri, T{(R) 1, (R) 0});
			// dst_bl = -dst_br * T       (== the reference's solve with src_br, :75-77)
			matmul_triangular_dev<T>(dst.sub(base + h, base, h2, h), 0, false, dst.sub(base + h, base + h, h2, h2).c(), tri, Tm.c(), 0,
						 T{(R) -1, (R) 0});
		}
}

} // namespace

void ctrtri_shape(int elem_bytes, size_t out[2])
{
	(void) elem_bytes; // c32 and c64 share the leaf's shape
	out[0] = E;
	out[1] = E / SB;
}

template <> void tri_invert_lower_dev<c32>(MatV<c32> dst, MatV<const c32> src, bool unit) { ctrtri_run<float>(dst, src, unit); }
template <> void tri_invert_lower_dev<c64>(MatV<c64> dst, MatV<const c64> src, bool unit) { ctrtri_run<double>(dst, src, unit); }

} // namespace fh

extern "C" FAER_HIP_API void faer_hip_debug_ctrtri_shape(int elem_bytes, size_t out[2]) { fh::ctrtri_shape(elem_bytes, out); }
