// One device allocation per call, handed out in aligned slices ("Scratch sites": the general EVD).
//
// The arena owns a single scratch buffer of the per-thread pool for the lifetime of the call; take<T>() carves 256-byte
// aligned slices off its front and aborts when the plan of the caller did not reserve enough.  Nothing is cleared: a slice
// holds whatever the pool's previous user left (or the fill byte of faer_hip_debug_scratch_fill), so every consumer writes
// before it reads.  copy_in / copy_out stage a host operand through a slice the way Staged does: one 2-D copy for a view with
// unit row (or column) stride, packing through a temporary host buffer for anything else.
#pragma once
#include "common.h"

namespace fh {

struct Arena {
	Scratch buf;
	size_t cap, off = 0;
	explicit Arena(size_t bytes) : buf(bytes), cap(bytes) {}
	static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t) 255; }
	template <typename T> T *take(size_t count)
	{
		const size_t bytes = padded(count * sizeof(T));
		FH_CHECK(off + bytes <= cap, "arena: the plan of the call is smaller than its slices");
		T *p = reinterpret_cast<T *>(static_cast<char *>(buf.p) + off);
		off += bytes;
		return p;
	}
	template <typename T> MatV<T> mat(idx_t nrows, idx_t ncols) { return MatV<T>{take<T>((size_t) nrows * (size_t) ncols), nrows, ncols, 1, nrows}; }

	// dense column-major device image of the host view v (its elements only)
	template <typename T> MatV<T> copy_in(MatV<const T> v)
	{
		MatV<T> d = mat<T>(v.nrows, v.ncols);
		if (v.nrows == 0 || v.ncols == 0)
			return d;
		hipStream_t s = ctx().stream;
		const idx_t pitch_limit = (idx_t) 1 << 30;
		if (v.rs == 1 && (v.cs >= v.nrows || v.ncols == 1) && v.cs * (idx_t) sizeof(T) < pitch_limit) {
			const idx_t hp = v.ncols == 1 ? v.nrows : v.cs;
			FH_HIP(hipMemcpy2DAsync(d.p, (size_t) v.nrows * sizeof(T), v.p, (size_t) hp * sizeof(T), (size_t) v.nrows * sizeof(T), (size_t) v.ncols,
						hipMemcpyHostToDevice, s));
			FH_HIP(hipStreamSynchronize(s));
			return d;
		}
		std::vector<T> pack((size_t) v.nrows * (size_t) v.ncols);
		for (idx_t j = 0; j < v.ncols; ++j)
			for (idx_t i = 0; i < v.nrows; ++i)
				pack[(size_t) (j * v.nrows + i)] = v.p[i * v.rs + j * v.cs];
		FH_HIP(hipMemcpyAsync(d.p, pack.data(), pack.size() * sizeof(T), hipMemcpyHostToDevice, s));
		FH_HIP(hipStreamSynchronize(s));
		return d;
	}
	// the dense column-major device matrix d back into the host view v (its elements only); synchronises the stream
	template <typename T> static void copy_out(MatV<T> v, MatV<const T> d)
	{
		if (v.nrows == 0 || v.ncols == 0)
			return;
		hipStream_t s = ctx().stream;
		const idx_t pitch_limit = (idx_t) 1 << 30;
		if (v.rs == 1 && (v.cs >= v.nrows || v.ncols == 1) && v.cs * (idx_t) sizeof(T) < pitch_limit) {
			const idx_t hp = v.ncols == 1 ? v.nrows : v.cs;
			FH_HIP(hipMemcpy2DAsync(v.p, (size_t) hp * sizeof(T), d.p, (size_t) d.cs * sizeof(T), (size_t) v.nrows * sizeof(T), (size_t) v.ncols,
						hipMemcpyDeviceToHost, s));
			FH_HIP(hipStreamSynchronize(s));
			return;
		}
		std::vector<T> pack((size_t) v.nrows * (size_t) v.ncols);
		FH_HIP(hipMemcpy2DAsync(pack.data(), (size_t) v.nrows * sizeof(T), d.p, (size_t) d.cs * sizeof(T), (size_t) v.nrows * sizeof(T),
					(size_t) v.ncols, hipMemcpyDeviceToHost, s));
		FH_HIP(hipStreamSynchronize(s));
		for (idx_t j = 0; j < v.ncols; ++j)
			for (idx_t i = 0; i < v.nrows; ++i)
				v.p[i * v.rs + j * v.cs] = pack[(size_t) (j * v.nrows + i)];
	}
};

} // namespace fh
