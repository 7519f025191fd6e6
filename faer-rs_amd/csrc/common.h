// Shared host-side infrastructure of libfaer_hip.so (gfx950 only, no compatibility layers).
//
//  * MatV<T>: the strided view every driver works on.  It is faer's MatView
//    {ptr, nrows, ncols, row_stride, col_stride} (faer/src/mat/mod.rs:7-13) with strides in elements.
//  * Ctx: per-thread device / stream / scratch state.  faer's entry points may be called from any
//    rayon worker => everything mutable is thread_local.
//  * Staged<T>: host<->device staging so that a host-resident faer::Mat works unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <atomic>
#include <vector>

#include "../../include/faer_hip.h"

namespace fh {

[[noreturn]] inline void die(const char *msg, const char *file, int line)
{
	fprintf(stderr, "faer_hip: fatal: %s (%s:%d)\n", msg, file, line);
	fflush(stderr);
	abort();
}
#define FH_CHECK(cond, msg)                                                                                             \
	do {                                                                                                            \
		if (!(cond))                                                                                            \
			::fh::die(msg, __FILE__, __LINE__);                                                             \
	} while (0)
#define FH_HIP(expr)                                                                                                    \
	do {                                                                                                            \
		hipError_t e_ = (expr);                                                                                 \
		if (e_ != hipSuccess)                                                                                   \
			::fh::die(hipGetErrorString(e_), __FILE__, __LINE__);                                           \
	} while (0)

typedef long idx_t;

// typed fused multiply-add: __builtin_fma is the DOUBLE builtin -- called with floats it converts to fp64 and back
// (three extra conversions per operation and the quarter-rate fp64 pipe); templates must use this overload pair
static __device__ __forceinline__ double fh_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
static __device__ __forceinline__ float fh_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// complex scalars of the boundary: faer's c32 / c64 are repr(C) {re, im}, interleaved (strides stay in complex elements).
// Level 3 (cgemm.hip, ctrsm.hip, ctrtri.hip) and the partial-pivot LU (cgetrf.hip) know them; everything else in the tree is instantiated for
// float / double.
template <typename R> struct Cx {
	R re, im;
};
typedef Cx<float> c32;
typedef Cx<double> c64;
template <typename T> struct is_cx : std::false_type {};
template <typename R> struct is_cx<Cx<R>> : std::true_type {};

template <typename T> struct MatV {
	T *p;
	idx_t nrows, ncols, rs, cs;

	MatV sub(idx_t r0, idx_t c0, idx_t nr, idx_t nc) const { return MatV{p + r0 * rs + c0 * cs, nr, nc, rs, cs}; }
	MatV t() const { return MatV{p, ncols, nrows, cs, rs}; }
	MatV rev_rows() const { return MatV{nrows > 0 ? p + (nrows - 1) * rs : p, nrows, ncols, -rs, cs}; }
	MatV rev_cols() const { return MatV{ncols > 0 ? p + (ncols - 1) * cs : p, nrows, ncols, rs, -cs}; }
	MatV<const T> c() const { return MatV<const T>{p, nrows, ncols, rs, cs}; }
};

// ------------------------------------------------------------------------------------------------
// per-thread context
// ------------------------------------------------------------------------------------------------
struct Ctx {
	int device = -1;
	hipStream_t stream = nullptr;
	int gemm_variant = 0;
	// scratch pool: simple stack of device buffers reused across calls of this thread
	struct Buf {
		void *p;
		size_t bytes;
		bool used;
		hipStream_t owner; // stream whose work last used the buffer: reuse is stream ordered only on that stream
	};
	std::vector<Buf> pool;
	int *host_ints = nullptr; // 16 pinned host ints: read-back target of the drivers that return a status per call
	int *pinned_ints();
	// Look-ahead execution (factorizations): two internal streams on DISJOINT sets of CUs
	// (hipExtStreamCreateWithCUMask): `la_bulk` runs the trailing-matrix GEMMs on most of the chip, `la_panel`
	// the latency-bound diagonal-block / panel work on a few reserved CUs, so neither queue can starve the other.
	hipStream_t la_bulk = nullptr, la_panel = nullptr;
	int la_state = 0; // 0: not tried, 1: available, -1: unavailable
	int la_panel_cus = 32;
	std::vector<hipEvent_t> la_events;
	size_t la_next_event = 0;
	bool lookahead_streams(); // creates the streams on first use; false if the runtime refuses
	// Plain side stream + events of the one-pass QR (tsqr.hip): ONE stream for both of its roles, created before the two
	// CU-masked streams above.  The runtime maps streams onto 4 hardware queues by default; as the 4th and 5th stream of the
	// process the QR's side streams made every kernel of the QR -- on the caller's stream too -- 1.3-6x slower (bench.py:
	// QR after an LLT in the same process 2.78 ms against 2.04; profiles/r03_qr_stream_order.txt).
	hipStream_t qr_side[2] = {nullptr, nullptr};
	hipEvent_t qr_ev[4] = {nullptr, nullptr, nullptr, nullptr};
	void qr_side_streams();
	hipEvent_t next_event();  // timing-disabled events, recycled per factorization (reset_events)
	void reset_events() { la_next_event = 0; }
	int ncu = 0;
	int stream_cus(); // compute units the current stream can occupy (the look-ahead streams are CU masked)
	// Kernel-class profile (faer_hip_prof_begin / faer_hip_prof_end, bench.py's per-workload `roofline`): while on, every launch
	// of a dominant kernel class is bracketed by two timing events on ITS stream; prof_end adds the spans up per class.
	// Classes: 0 big-tile MFMA products (units: flop), 1 LU panel kernel (columns), 2 one-pass QR update (algorithmic bytes),
	// 3 one-pass QR Gram (bytes), 4 one-pass QR panel kernel (launches), 5 Cholesky leaf (columns).
	struct ProfSpan {
		hipEvent_t a, b;
		int cls;
		double units;
		long d[4] = {0, 0, 0, 0}; // class 0: m, n, k of the product, 1 + tri_skip for a Lower destination (0: Full)
		int sid = 0;		  // 0 caller's stream, 1 bulk, 2 panel, 3 side
	};
	static constexpr int PROF_CLASSES = 6;
	bool prof_on = false;
	std::vector<ProfSpan> prof_spans;
	std::vector<hipEvent_t> prof_pool;
	hipEvent_t prof_event();

	void ensure_device();
	void *alloc(size_t bytes); // returns a device buffer valid until release()
	void release(void *p);
	void sync() { FH_HIP(hipStreamSynchronize(stream)); }
	void set_stream(hipStream_t s); // the caller's stream (faer_hip_set_stream); internal code switches `stream` directly
	// after a point where every internal stream has been joined AND the caller's stream synchronised: free
	// buffers last used on these streams may be handed to any stream again (those of other caller streams keep their owner).
	// What that costs: a free buffer whose owner is a caller stream that was still busy when set_stream() left it is not polled
	// again (alloc() polls the library's own streams and the null stream only, set_stream() the stream it leaves -- a stream the
	// caller may have destroyed must not be queried); it is reused when the caller returns to that stream, else it stays in the pool
	// until a failed hipMalloc purges the free buffers.  A caller cycling through short-lived streams with work in flight grows
	// the pool by up to one set of buffers per stream.
	void quiesce();
};
Ctx &ctx();

// Raises Kernel's dynamic LDS limit once per DEVICE and kernel: the attribute belongs to the device that is current at the
// time of the call, and a thread bound to a second GPU must not launch without it (atomic flags: several threads; a device
// number past the 64 bits sets it on every call).
template <auto Kernel> inline void raise_dynamic_lds(size_t bytes)
{
	static std::atomic<unsigned long long> attr_done{0}; // bit d: device d
	const int dev = ctx().device;
	const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
	if (bit == 0 || !(attr_done.load(std::memory_order_acquire) & bit)) {
		FH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes));
		attr_done.fetch_or(bit, std::memory_order_release);
	}
}
void debug_stream_xcc(int which, int nblocks, unsigned *out_host); // which: 0 caller's stream, 1 bulk, 2 panel
void prof_collect(double *out, double *spans = nullptr, size_t cap = 0, size_t *nspans = nullptr); // Ctx::PROF_CLASSES x {ms, launches, units} of the spans recorded since prof_on; optionally one record of 8 doubles per span (ctx.hip)
double xwg_hop_us(int iters); // idle-chip hand-off latency between two workgroups, microseconds (ctx.hip)
void debug_scratch_fill(int byte_or_minus_one); // debug: every scratch buffer handed out is filled with this byte first (-1 = off, the default; ctx.hip)
void debug_scratch_fill_stats(size_t out[2]);  // {fills, bytes filled} since the last debug_scratch_fill
void ctx_shutdown(); // releases the calling thread's look-ahead streams / events, pinned ints and free scratch buffers (the context stays usable); safe without a device

// stream `s` waits for event `e`
inline void stream_wait(hipStream_t s, hipEvent_t e) { FH_HIP(hipStreamWaitEvent(s, e, 0)); }

// RAII: run the enclosed launches on another stream
struct StreamScope {
	hipStream_t saved;
	explicit StreamScope(hipStream_t s) : saved(ctx().stream) { ctx().stream = s; }
	~StreamScope() { ctx().stream = saved; }
	StreamScope(const StreamScope &) = delete;
	StreamScope &operator=(const StreamScope &) = delete;
};

// RAII: one profiled launch (no-op unless Ctx::prof_on)
struct ProfScope {
	Ctx::ProfSpan sp;
	bool on;
	ProfScope(int cls, double units) : on(ctx().prof_on && cls >= 0)
	{
		if (!on)
			return;
		sp.cls = cls;
		sp.units = units;
		{
			Ctx &c = ctx();
			sp.sid = c.stream == c.la_bulk ? 1 : (c.stream == c.la_panel ? 2 : (c.qr_side[0] && c.stream == c.qr_side[0] ? 3 : 0));
		}
		sp.a = ctx().prof_event();
		sp.b = ctx().prof_event();
		FH_HIP(hipEventRecord(sp.a, ctx().stream));
	}
	~ProfScope() // may run while an exception unwinds: never throws, a span whose end cannot be recorded is dropped
	{
		if (!on)
			return;
		if (hipEventRecord(sp.b, ctx().stream) != hipSuccess) {
			(void) hipGetLastError();
			sp.cls = -1;
		}
		try {
			ctx().prof_spans.push_back(sp);
		} catch (...) {
		}
	}
	ProfScope(const ProfScope &) = delete;
	ProfScope &operator=(const ProfScope &) = delete;
};

// RAII scratch
struct Scratch {
	void *p;
	explicit Scratch(size_t bytes) : p(ctx().alloc(bytes)) {}
	~Scratch() { ctx().release(p); }
	Scratch(const Scratch &) = delete;
	Scratch &operator=(const Scratch &) = delete;
	template <typename T> T *as() const { return static_cast<T *>(p); }
};

bool is_device_ptr(const void *p);

// Span of memory (in elements, relative to .p) touched by a strided view.
template <typename T> inline void view_span(const MatV<T> &v, idx_t &lo, idx_t &hi)
{
	lo = 0;
	hi = 0;
	if (v.nrows == 0 || v.ncols == 0)
		return;
	idx_t r = (v.nrows - 1) * v.rs, c = (v.ncols - 1) * v.cs;
	lo = (r < 0 ? r : 0) + (c < 0 ? c : 0);
	hi = (r > 0 ? r : 0) + (c > 0 ? c : 0);
}

// Host->device staging of one operand.  If the view already lives in device memory it is used in place;
// otherwise EXACTLY the elements of the view are copied into a dense device buffer (and copied back on
// destruction when `writeback` is set).  The gaps of a strided host view -- the parent matrix's entries between
// the columns of a `submatrix_mut`, which other rayon workers may be writing at the same time -- are never read
// and never written (round 1 staged the whole contiguous span and wrote it back, gaps included).
//   * unit row stride, positive column stride (a faer::Mat or a block of one): one hipMemcpy2DAsync, column major;
//   * unit column stride, positive row stride (a transposed view): the same, row major;
//   * anything else (negative / non-unit strides): packed through a temporary host buffer.
template <typename T> struct Staged {
	typedef typename std::remove_const<T>::type U;
	MatV<T> dev;
	MatV<T> host;
	void *buf = nullptr;
	U *pack = nullptr; // host-side packing buffer (mode 3)
	int mode = 0;	   // 0: device operand, 1: column-major 2-D copy, 2: row-major 2-D copy, 3: host packed (column major)
	bool writeback = false;

	// host pitch (elements) of the 2-D copy; a single column / row may carry any outer stride (even 0)
	idx_t hpitch() const
	{
		if (mode == 1)
			return host.ncols == 1 ? host.nrows : host.cs;
		return host.nrows == 1 ? host.ncols : host.rs;
	}

	Staged(MatV<T> v, bool copy_in, bool writeback_)
	{
		dev = v;
		host = v;
		if (v.nrows == 0 || v.ncols == 0 || is_device_ptr(v.p))
			return;
		const size_t bytes = (size_t) v.nrows * (size_t) v.ncols * sizeof(T);
		buf = ctx().alloc(bytes);
		writeback = writeback_;
		const idx_t pitch_limit = (idx_t) 1 << 30; // bytes; beyond it (never for a real Mat) fall back to packing
		if (v.rs == 1 && (v.cs >= v.nrows || v.ncols == 1) && v.cs * (idx_t) sizeof(T) < pitch_limit) {
			mode = 1;
			dev = MatV<T>{static_cast<T *>(buf), v.nrows, v.ncols, 1, v.nrows};
		} else if (v.cs == 1 && (v.rs >= v.ncols || v.nrows == 1) && v.rs * (idx_t) sizeof(T) < pitch_limit) {
			mode = 2;
			dev = MatV<T>{static_cast<T *>(buf), v.nrows, v.ncols, v.ncols, 1};
		} else {
			mode = 3;
			dev = MatV<T>{static_cast<T *>(buf), v.nrows, v.ncols, 1, v.nrows};
			pack = static_cast<U *>(malloc(bytes));
			FH_CHECK(pack != nullptr, "staging: out of host memory");
		}
		if (!copy_in)
			return;
		if (mode == 1) {
			FH_HIP(hipMemcpy2DAsync(buf, (size_t) v.nrows * sizeof(T), (const void *) v.p, (size_t) hpitch() * sizeof(T),
						(size_t) v.nrows * sizeof(T), (size_t) v.ncols, hipMemcpyHostToDevice, ctx().stream));
		} else if (mode == 2) {
			FH_HIP(hipMemcpy2DAsync(buf, (size_t) v.ncols * sizeof(T), (const void *) v.p, (size_t) hpitch() * sizeof(T),
						(size_t) v.ncols * sizeof(T), (size_t) v.nrows, hipMemcpyHostToDevice, ctx().stream));
		} else {
			for (idx_t j = 0; j < v.ncols; ++j)
				for (idx_t i = 0; i < v.nrows; ++i)
					pack[j * v.nrows + i] = v.p[i * v.rs + j * v.cs];
			FH_HIP(hipMemcpyAsync(buf, pack, bytes, hipMemcpyHostToDevice, ctx().stream));
			FH_HIP(hipStreamSynchronize(ctx().stream)); // `pack` is reused by the write-back
		}
	}
	~Staged()
	{
		if (!buf)
			return;
		if (writeback) {
			U *hp = const_cast<U *>(host.p);
			if (mode == 1) {
				FH_HIP(hipMemcpy2DAsync((void *) hp, (size_t) hpitch() * sizeof(T), buf, (size_t) host.nrows * sizeof(T),
							(size_t) host.nrows * sizeof(T), (size_t) host.ncols, hipMemcpyDeviceToHost, ctx().stream));
				FH_HIP(hipStreamSynchronize(ctx().stream));
			} else if (mode == 2) {
				FH_HIP(hipMemcpy2DAsync((void *) hp, (size_t) hpitch() * sizeof(T), buf, (size_t) host.ncols * sizeof(T),
							(size_t) host.ncols * sizeof(T), (size_t) host.nrows, hipMemcpyDeviceToHost, ctx().stream));
				FH_HIP(hipStreamSynchronize(ctx().stream));
			} else {
				FH_HIP(hipMemcpyAsync(pack, buf, (size_t) host.nrows * (size_t) host.ncols * sizeof(T), hipMemcpyDeviceToHost,
						      ctx().stream));
				FH_HIP(hipStreamSynchronize(ctx().stream));
				for (idx_t j = 0; j < host.ncols; ++j)
					for (idx_t i = 0; i < host.nrows; ++i)
						hp[i * host.rs + j * host.cs] = pack[j * host.nrows + i];
			}
		}
		free(pack);
		ctx().release(buf);
	}
	Staged(const Staged &) = delete;
	Staged &operator=(const Staged &) = delete;
};

// ------------------------------------------------------------------------------------------------
// device-level drivers (operands are device memory); defined in the .hip files
// ------------------------------------------------------------------------------------------------
enum DstKind { DST_FULL = 0, DST_LOWER = 1, DST_UPPER = 2 };

template <typename T> struct GemmExtra {
	const void *row_idx = nullptr; // device memory, itype-wide indices
	const void *col_idx = nullptr;
	int idx64 = 1;
	const T *diag = nullptr; // device memory
	idx_t diag_stride = 0;
	int a_struct = 0, b_struct = 0; // FaerBlock codes of the operands (triangular products)
	bool dst_strict = false;	// with DST_LOWER / DST_UPPER: leave the diagonal untouched
	// dense-kernel shortcuts for the factorization drivers (plain products only):
	//   k_trim 1: rhs(k, n) is zero for k > n (upper triangular rhs with an explicitly zeroed lower part), 2: lhs(m, k)
	//   is zero for k > m -- each tile stops its K loop at the end of its diagonal block instead of multiplying zeros;
	//   tri_skip (DST_LOWER, square): the first `tri_skip` rows of the lower triangle (a multiple of 128) are left
	//   untouched, i.e. one launch covers "block column below the leading block + remaining lower square".
	//   stair_nb / stair_gap (DST_LOWER, any shape): the "diagonal" is a staircase -- column n of dst stands for column
	//   n + (n / stair_nb) * stair_gap of the matrix it is a part of (the owned block columns of a 1-D block-cyclic
	//   partition next to each other: dist_llt.h), entries above it are left untouched.  stair_row0: row 0 of dst is row
	//   stair_row0 of that picture (a row chunk of the staircase: dst(i, n) is written iff i + stair_row0 >= that column).
	int k_trim = 0;
	idx_t tri_skip = 0;
	idx_t stair_nb = 0, stair_gap = 0, stair_row0 = 0;
	// short-wide / tall-narrow FULL output with a deep K (the V^H A product of a QR block application, 128 x n with K = rows): 128 x 128
	// tiles with more K slices instead of the 64 x 64 tiles the tile-count rule picks (square QR N = 8192: -3 %, tools/gpu_qr_square_gemm_ab.py)
	bool prefer_big_tiles = false;
	// complex scalars only (cgemm.hip): op(lhs) / op(rhs) is the conjugate (the real kernels never look at these)
	bool conj_lhs = false, conj_rhs = false;
};

// Ctx::gemm_variant (faer_hip_set_gemm_variant): the integers are public, tools and tests pass them through
enum GemmVariant {
	GEMM_VARIANT_AUTO = 0,	      // the rules of gemm_plan
	GEMM_VARIANT_FORCE_128 = 1,   // pipelined 128 x 128 tile
	GEMM_VARIANT_FORCE_64 = 2,    // pipelined 64 x 64 tile
	GEMM_VARIANT_FORCE_WIDE = 3,  // pipelined 128 x 256 tile wherever it can run (plain full and square lower products)
	GEMM_VARIANT_NO_WIDE = 5,     // auto without the 128 x 256 tile
	GEMM_VARIANT_DEEP_K_BIG = 6,  // GemmExtra::prefer_big_tiles for every product
	GEMM_VARIANT_LEGACY = 10,     // from here up: the non-pipelined kernel (k_trim / tri_skip / stair_nb are refused)
	GEMM_VARIANT_LEGACY_128 = 11, // non-pipelined 128 x 128 tile
	GEMM_VARIANT_LEGACY_64 = 12,  // non-pipelined 64 x 64 tile
};

// The dense dispatch of gemm_dev as data (gemm.hip: gemm_orient, gemm_plan): pure host integer logic, no device needed
// (faer_hip_debug_gemm_plan).  GemmProblem is a product past the level-2 exits, in elements and element strides.
struct GemmProblem {
	idx_t m, n, k;
	int elem_bytes;
	DstKind kind;
	bool add;
	int alpha_sign; // 1: alpha == 1, -1: alpha == -1, 0: any other value
	idx_t drs, dcs, ars, acs, brs, bcs;
	bool indexed, diag; // GemmExtra::row_idx or col_idx / diag given
	int a_struct, b_struct, k_trim;
	idx_t tri_skip, stair_nb, stair_gap, stair_row0;
	bool prefer_big_tiles;
	int variant;
	bool transposed; // set by gemm_orient
};
enum GemmTile {
	GEMM_TILE_EXTRA64 = 0, // gemm_kernel<EXTRA>: structured operands, diag scaling
	GEMM_TILE_PIPE64 = 1,  // gemm_kernel_p
	GEMM_TILE_PIPE128 = 2,
	GEMM_TILE_PIPE_WIDE = 3, // 128 x 256, eight wavefronts
	GEMM_TILE_LEGACY64 = 4,	 // gemm_kernel: pointer-addressed loaders, any strides
	GEMM_TILE_LEGACY128 = 5,
};
struct GemmPlan {
	bool transposed;
	bool tri_skip_split; // tri_skip on operands the pipelined loaders cannot address: two plain products (only akm, bkm, routes set besides)
	GemmTile tile;
	bool akm, bkm;	  // K-major loaders
	int bm, bn, ntm, ntn;
	int tri_enum, tri_off;
	int splits, k_per_split;
	int fast_io;
	int prof_class;
	unsigned routes; // bit r: FaerHipRoute r counts once for this launch
};
bool gemm_orient(GemmProblem &p);				  // puts the problem into the orientation the kernels run; true if it transposed
const char *gemm_plan(const GemmProblem &p, GemmPlan &plan); // nullptr, or why the product is refused (gemm_dev aborts with it)

// route counters of the GEMM / TRSM dispatch (faer_hip_debug_route_counts): thread-local, defined in gemm.hip
extern thread_local long long g_route_counts[FaerHipRoute_Count];
static inline void route_hit(FaerHipRoute r) { ++g_route_counts[r]; }

// dst(kind) <- [dst +] alpha * A * diag * B        (gemm.hip)
template <typename T>
void gemm_dev(MatV<T> C, DstKind kind, bool add, MatV<const T> A, MatV<const T> B, T alpha,
	      const GemmExtra<T> *extra = nullptr);
// level-2 shapes (gemv.hip): matrix-vector product and rank-1 update, HBM streams outside the MFMA kernel
template <typename T> bool gemv_dev(idx_t m, idx_t k, MatV<const T> A, const T *x, idx_t xs, T *y, idx_t ys, T alpha, bool add);
template <typename T> void rank1_dev(MatV<T> C, bool add, const T *a, idx_t as, const T *b, idx_t bs, T alpha);
// extras.hip / trsm.hip: triangular inverse (triangular_inverse.rs) and helpers of the reconstruct / inverse entry points
template <typename T> void tri_invert_lower_dev(MatV<T> dst, MatV<const T> src, bool unit);
template <typename T> void ldlt_scale_lower_dev(MatV<T> out, MatV<const T> L, const T *d, idx_t ds);
template <typename T> void ldlt_inverse_prepare_dev(MatV<T> W, const T *d, idx_t ds);
template <typename T> void zero_then_upper_dev(MatV<T> out, const MatV<const T> *R);
// fplu.hip: LU with full pivoting (perm arrays are host memory); returns the transposition count
void fplu_debug_inplace(int on); // fplu.hip: 1 = the in-place two-launch path (A/B tests)
template <typename T> long full_piv_lu_dev(MatV<T> A, idx_t *row_perm, idx_t *row_perm_inv, idx_t *col_perm, idx_t *col_perm_inv);
// colpiv_qr.hip: QR with column pivoting (perm arrays are host memory); returns the transposition count
template <typename T> long colpiv_qr_dev(MatV<T> A, MatV<T> H, idx_t *col_perm, idx_t *col_perm_inv);
// pure host planning logic, exported for the CPU tests (faer_hip_debug_*)
std::vector<idx_t> llt_plan(idx_t n, idx_t tail_rows, idx_t nb2);
size_t llt_debug_steps(idx_t n, idx_t la_min, idx_t tail_rows, idx_t side_rmin, idx_t dpanel_rmin, int *codes, size_t cap);
int lu_leaf_width(idx_t m, int elem_bytes, int resident_workgroups);
bool dist_two_streams_ok(idx_t panel_rows, int elem_bytes, int panel_cus, int all_cus);
void lu_force_general(int on); // debug: every LU leaf on the non-cooperative path
void lu_debug_plan(long nb2_from, long pipe_from, long la_min); // debug: switch-over points of the look-ahead LU driver (0 = default)
void lu_lend_copy(const void *device_copy, idx_t nrows, idx_t ncols, int elem_bytes); // the calling thread's next LU may restore A from it after an exchange timeout (getrf.hip)
bool rccl_is_builtin_wait(FaerHipWaitFn fn); // rccl_transport.hip: is this the built-in transport's wait (takes any stream)
bool loop_is_builtin_wait(FaerHipWaitFn fn); // loop_transport.hip: the loop-back transport of the tests (ranks = threads on one GPU)
void level2_debug_force_memory_bodies(int on); // debug: tridiag / bidiag / Hessenberg vector kernels never keep their columns in registers
void tsqr_debug_panel_copy(int on); // debug: 0 = the fp32 one-pass QR never keeps a raw copy of the panel (the path of matrices of more than 4.19 M rows), 1 = where it fits (default)
void tsqr_debug_f64(int on); // debug: 0 = fp64 matrices never take the one-pass QR path
void tsqr_debug_shape_rule(long min_rows, long min_aspect); // debug: shape rule of the whole-matrix one-pass QR path (0 = default)
void tsqr_debug_panels(int on); // debug: 0 = the classic QR path never factors a panel on the one-pass path
long qr_last_one_pass_columns(); // debug: columns the one-pass QR path completed in this thread's last factorization (-1: not taken)
// tall-skinny shapes (skinny.hip): streaming kernels; false if the shape / strides do not qualify
template <typename T> bool skinny_dev(MatV<T> C, bool add, MatV<const T> A, MatV<const T> B, T alpha);
// C <- [C +] alpha * sum_z ws[z] (slices of nrows x ncols, column major), fixed summation order (gemm.hip)
template <typename T> void splitk_reduce_dev(MatV<T> C, const T *ws, int splits, T alpha, bool add);
// average ms per launch of the dense kernel (hipEvents on the ctx stream)
template <typename T> double gemm_time_ms(MatV<T> C, MatV<const T> A, MatV<const T> B, int iters);
double mfma_peak_tflops(bool f64, int iters);

// dst(structure) <- [dst +] alpha * A(structure) * B(structure)   (trmm.hip)
template <typename T>
void matmul_triangular_dev(MatV<T> C, int c_s, bool add, MatV<const T> A, int a_s, MatV<const T> B, int b_s, T alpha);

// complex scalars (cgemm.hip): the same two drivers on the complex MFMA kernel.  GemmExtra::conj_lhs / conj_rhs are honoured, all seven
// FaerBlock kinds and the three DstKinds are masked loads / stores of that one kernel; row_idx / col_idx / diag are refused.  No workspace.
template <> void gemm_dev<c32>(MatV<c32> C, DstKind kind, bool add, MatV<const c32> A, MatV<const c32> B, c32 alpha, const GemmExtra<c32> *extra);
template <> void gemm_dev<c64>(MatV<c64> C, DstKind kind, bool add, MatV<const c64> A, MatV<const c64> B, c64 alpha, const GemmExtra<c64> *extra);
template <> void matmul_triangular_dev<c32>(MatV<c32> C, int c_s, bool add, MatV<const c32> A, int a_s, MatV<const c32> B, int b_s, c32 alpha);
template <> void matmul_triangular_dev<c64>(MatV<c64> C, int c_s, bool add, MatV<const c64> A, int a_s, MatV<const c64> B, int b_s, c64 alpha);
// complex scalars (ctrtri.hip): the recursion of extras.hip on an LDS-resident complex leaf and the two drivers above
template <> void tri_invert_lower_dev<c32>(MatV<c32> dst, MatV<const c32> src, bool unit);
template <> void tri_invert_lower_dev<c64>(MatV<c64> dst, MatV<const c64> src, bool unit);
void ctrtri_shape(int elem_bytes, size_t out[2]); // {E: edge of a leaf, sub-blocks along that edge}; elem_bytes 8 (c32) or 16 (c64)

// X <- op(T)^-1 X, T lower triangular n x n, X n x k (trsm.hip); upper handled by reversal
template <typename T> void trsm_lower_dev(MatV<const T> L, bool unit, MatV<T> X);
template <typename T> void trsm_upper_dev(MatV<const T> U, bool unit, MatV<T> X);
// complex scalars (ctrsm.hip): X <- op(T)^-1 X with op the identity or the conjugate; blocked substitution, the updates on gemm_dev<Cx<R>>
template <typename R> void ctrsm_dev(MatV<const Cx<R>> T, bool upper, bool unit, bool conj, MatV<Cx<R>> X);
idx_t ctrsm_leaf_rows(); // rows of the diagonal blocks the substitution kernel solves
// same as trsm_lower_dev with the packed images (trsm_pack.h) of L's 128 x 128 diagonal blocks already in W
template <typename T> void trsm_lower_pre_dev(MatV<const T> L, MatV<T> X, const T *W);
template <typename T> void trsm_pack_dev(MatV<const T> L, bool unit, T *W);
void trsm_dump_timing(); // timing build only (no-op otherwise)
void lu_dump_timing();   // timing build only: per-phase ticks of the LU panel kernel (getrf.hip)
void gemm_dump_timing(); // timing build only: per-phase ticks of the pipelined GEMM tile (gemm.hip)

// in-place lower Cholesky; returns >=0 regularization count or -(index+1)   (potrf.hip)
template <typename T> long potrf_lower_dev(MatV<T> A, T reg_delta, T reg_eps);
template <typename T> void potrf_panel_dev(MatV<T> P, T reg_delta, T reg_eps, int *status_dev, idx_t offset);

// in-place unit-lower L D L^T without pivoting (potrf.hip); L strictly below the diagonal, D on it; `signs_host`: n int8
// expected pivot signs or NULL; returns >= 0 regularization count or -(index + 1) of the zero pivot
template <typename T> long sytrf_lower_dev(MatV<T> A, T reg_delta, T reg_eps, const signed char *signs_host);

// partial pivot LU; perm/perm_inv are HOST arrays of idx_t (m entries)   (getrf.hip)
template <typename T> long getrf_dev(MatV<T> A, idx_t *perm, idx_t *perm_inv);
// complex scalars (cgetrf.hip): the reference's recursion on panels of W columns; pivots by abs1 = |re| + |im|.  Never returns < 0.
template <> long getrf_dev<c32>(MatV<c32> A, idx_t *perm, idx_t *perm_inv);
template <> long getrf_dev<c64>(MatV<c64> A, idx_t *perm, idx_t *perm_inv);
void clu_shape(int elem_bytes, size_t out[2]); // {W, rows of the tallest panel the LDS leaf takes}; elem_bytes 8 (c32) or 16 (c64)
void clu_last(size_t out[4]); // {panels on the LDS leaf, panels on the column-step kernels, column-step launches, interchange launches} of the calling thread's last complex LU

// pieces of the LU driver used by the distributed driver (dist.hip): in-place factorization of an m x w panel
// (w <= m) with the pivots left on the device (piv_dev[j] = row swapped with row j, relative to the panel), and
// the application of such a transposition list to the rows of another block
template <typename T> void getrf_panel_dev(MatV<T> P, int *piv_dev, int *status_dev = nullptr);
template <typename T> void laswp_rows_dev(MatV<T> B, const int *piv_dev, int nt);
int laswp_list_max(); // most interchanges one composed list holds
void laswp_compose_rows_dev(const int *piv_dev, int nt, int *list_4nt); // net permutation of (j <-> piv[j]), j < nt, composed once ...
template <typename T> void laswp_list_rows_dev(MatV<T> B, const int *list_4nt, int nt); // ... and applied to any number of column ranges

// Householder QR without pivoting (qr.hip); H is block_size x min(m,n) (device). returns rank
template <typename T> long geqrf_dev(MatV<T> A, MatV<T> H, idx_t blocking_threshold);
// the T blocks of H (block_size x min(m, n)) over the first `rank` reflectors of A from their taus (device), the columns from `rank` on
// in the reference's zero / +inf pattern (qr.hip); the last step of every Householder-based driver
template <typename T> void qr_t_blocks_from_taus(MatV<T> A, MatV<T> H, idx_t rank, const T *taus);
// The one-pass QR path (tsqr.hip; float: fused schedule, double: plain schedule) for whole tall matrices (geqrf_dev) and for single
// panels / two-panel nodes of the classic recursion (qr_rec).  tsqr_factor returns the number of COLUMNS completed, `reason` says
// why it stopped early; `rows_above`: rows of a parent matrix above A that count in the reference's rank test.
template <typename T> bool tsqr_applicable(MatV<T> A, idx_t bs);
template <typename T> bool tsqr_panel_applicable(idx_t m, idx_t w, idx_t rs, idx_t cs);
template <typename T> idx_t tsqr_factor(MatV<T> A, MatV<T> H, T *taus, int *reason, idx_t rows_above = 0);
template <> idx_t tsqr_factor<float>(MatV<float> A, MatV<float> H, float *taus, int *reason, idx_t rows_above);
template <> idx_t tsqr_factor<double>(MatV<double> A, MatV<double> H, double *taus, int *reason, idx_t rows_above);
// evd/tridiag.rs:274: A (self-adjoint, lower triangle used) -> T + reflectors, H: block Householder factors (condense.hip)
template <typename T> void tridiag_dev(MatV<T> A, MatV<T> H);
// svd/bidiag.rs:47: A -> upper bidiagonal + reflectors, Hl / Hr: block Householder factors (condense.hip)
template <typename T> void bidiag_dev(MatV<T> A, MatV<T> Hl, MatV<T> Hr);
// evd/hessenberg.rs:549: A -> upper Hessenberg + reflectors, H: block Householder factors (condense.hip)
template <typename T> void hessenberg_dev(MatV<T> A, MatV<T> H);
template <typename T>
void apply_householder_sequence_left_dev(MatV<const T> V, MatV<const T> H, MatV<T> M, bool transpose);

// evd/mod.rs:270 self_adjoint_evd (evd.hip): S (n entries, stride ss, device) <- ascending eigenvalues of the self-adjoint A
// (lower triangle read), U (n x n, device) <- eigenvectors unless U.p == nullptr.  Leaves of the divide and conquer have at
// most `leaf` rows (evd_leaf_size), `bs` is the block size of the tridiagonalization's Householder factors.  Returns 0, or 1
// for NoConvergence (a non-finite tridiagonal or a leaf over its iteration cap).
idx_t evd_leaf_size(size_t recursion_threshold);
template <typename T> int self_adjoint_evd_dev(MatV<const T> A, MatV<T> U, T *S, idx_t ss, idx_t leaf, idx_t bs);
// svd/mod.rs:530 svd (svd.hip): S (min(m, n) entries, stride ss, device) <- nonincreasing singular values of A (m x n, never
// written), U (m x min(m, n) or m x m) / V (n x min(m, n) or n x n) <- singular vectors unless their .p == nullptr.  A wide
// matrix runs as its transpose with U and V swapped; a tall one with m / n > qr_ratio_threshold goes through geqrf_dev first.
// Leaves of the bidiagonal divide and conquer have at most `leaf` entries (svd_leaf_size); bs_mn / bs_nn: block sizes of the
// Householder factors of the max(m, n) x min(m, n) reduction and of the square one behind the QR pre-step.  Returns 0, or 1
// for NoConvergence (a non-finite bidiagonal form or a leaf over its iteration cap).
idx_t svd_leaf_size(size_t recursion_threshold);
template <typename T> void svd_identity_dev(MatV<T> X); // zero, ones on the diagonal (mod.rs:586-591)
template <typename T>
int svd_dev(MatV<const T> A, MatV<T> U, MatV<T> V, T *S, idx_t ss, idx_t leaf, double qr_ratio_threshold, idx_t qr_blocking_threshold,
	    idx_t bs_mn, idx_t bs_nn);

// evd/mod.rs:1007 evd_imp, real matrices (schur.hip): wr / wi (n contiguous device entries) <- real and imaginary parts of the
// eigenvalues of A (n x n, never written), UL / UR (n x n, device) <- left / right eigenvectors in the reference's packed layout
// unless their .p == nullptr.  All device memory comes from slices of `arena` (arena.h; evd_arena_bytes sizes it);
// a_is_arena_dense: A is a dense column-major slice the call may overwrite (a staged host operand).  bs: block size of the
// Hessenberg reduction's Householder factors; shift_count: FaerSchurParams::recommended_shift_count.  Returns 0, or 1 for
// NoConvergence (a non-finite entry of A, or the iteration cap).
struct Arena;
idx_t schur_window_edge(int elem_bytes);
size_t evd_arena_bytes(idx_t n, bool vectors, idx_t bs, int elem_bytes);
void evd_last_counts(long out[4]); // {sweeps, window steps, leaf launches, state read-backs} of the calling thread's last evd
template <typename T>
int evd_dev(Arena &arena, MatV<const T> A, bool a_is_arena_dense, MatV<T> UL, MatV<T> UR, T *wr, T *wi, idx_t bs, size_t (*shift_count)(size_t, size_t));

// gevd/mod.rs:130 gevd_real (qz.hip): alpha_re / alpha_im / beta (n contiguous device entries each) <- the eigenvalues
// (alpha_re + i alpha_im) / beta of the pair (A, B) (n x n, never written), UL / UR as in evd_dev.  All device memory comes from
// slices of `arena` (gevd_arena_bytes sizes it).  bs: block size of the QR of B.  Returns 0, or 1 for NoConvergence.
idx_t gevd_window_edge(int elem_bytes);
size_t gevd_arena_bytes(idx_t n, bool vectors, idx_t bs, int elem_bytes);
void gevd_last_counts(long out[5]); // {sweeps, window steps, QZ launches, state read-backs, infinite deflations} of the last call
template <typename T>
int gevd_dev(Arena &arena, MatV<const T> A, MatV<const T> B, MatV<T> UL, MatV<T> UR, T *alpha_re, T *alpha_im, T *beta, idx_t bs, idx_t qr_blocking_threshold,
	     size_t (*shift_count)(size_t, size_t));

// cholesky/llt/update.rs:360 and cholesky/ldlt/update.rs:376 rank_r_update_clobber (chol_update.hip): the factor in the lower triangle
// of L (n x n) becomes that of A + W diag(alpha) W^T; W (n x r) and alpha (r x 1) are clobbered.  Each operand is host or device
// memory on its own; all device memory of the call is one arena.  Returns -1, or the column of the non positive pivot (LLT).
template <typename T> long chol_rank_update(MatV<T> L, MatV<T> W, MatV<T> alpha, bool ldlt);
// cholesky/ldlt/update.rs:417 delete_rows_and_cols_clobber: idx holds r >= 1 strictly increasing indices below n (host memory)
template <typename T> void ldlt_delete_rows_and_cols(MatV<T> LD, const idx_t *idx, idx_t r);
void chol_update_last(long out[4]); // {column blocks, tail launches, chunks of W per block, host synchronisations inside the block loop} of the last call
void chol_update_shape(int elem_bytes, size_t out[2]); // {NB, RC}
void chol_update_debug_diag_only(int on); // measurement aid: 1 = only the diagonal kernels run (the chain of the call; the result is wrong)

// small utility kernels (util.hip)
template <typename T> void fill_dev(MatV<T> A, DstKind kind, T value);
template <typename T> void copy_dev(MatV<T> dst, MatV<const T> src);
template <typename T> void gather_rows_dev(MatV<T> dst, MatV<const T> src, const idx_t *perm_dev); // dst[i,:] = src[perm[i],:]
template <typename T> void scale_rows_recip_dev(MatV<T> X, const T *d, idx_t ds);		       // X[i,:] *= 1 / d[i]

} // namespace fh
