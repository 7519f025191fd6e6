// Device helpers shared by the Householder-based factorizations (qr.hip, colpiv_qr.hip, condense.hip): limits of the scalar
// types, the scaled norm of reductions/norm_l2.rs, and the wavefront / workgroup sums.
#pragma once
#include <hip/hip_runtime.h>

namespace fh {

template <typename T> struct Lim;
template <> struct Lim<double> {
	static constexpr double eps = 2.220446049250313e-16, minpos = 2.2250738585072014e-308;
};
template <> struct Lim<float> {
	static constexpr float eps = 1.1920929e-07f, minpos = 1.17549435e-38f;
};

template <typename T> static __device__ __forceinline__ double scale_sml() { return sqrt((double) Lim<T>::minpos); }
template <typename T> static __device__ __forceinline__ double scale_big() { return sqrt(1.0 / (double) Lim<T>::minpos); }

template <typename T> static __device__ T norm_from3(const double *acc)
{
	// reductions/norm_l2.rs:173-184
	const T sml = (T) scale_sml<T>(), big = (T) scale_big<T>();
	const T a0 = (T) acc[0], a1 = (T) acc[1], a2 = (T) acc[2];
	if (a0 >= (T) 1)
		return sqrt(a0) * big;
	if (a1 >= (T) 1)
		return sqrt(a1);
	return sqrt(a2) * sml;
}

static __device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1)
		v += __shfl_xor(v, off, 64);
	return v;
}

// sums vals[0 .. CNT) over the NT threads of the workgroup into s_red[0 .. CNT) (every thread may read s_red afterwards): wave sums, then
// CNT threads add the NT / 64 wave partials of s_part in wave order, starting FROM partial 0 (a sum of -0.0s stays -0.0)
template <int NT, int CNT> static __device__ __forceinline__ void block_sum(double (&vals)[CNT], double *s_part, double *s_red)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
	for (int c = 0; c < CNT; ++c) {
		const double s = wave_sum(vals[c]);
		if (lane == 0)
			s_part[wave * CNT + c] = s;
	}
	__syncthreads();
	if (tid < CNT) {
		double t = s_part[tid];
#pragma unroll
		for (int k = 1; k < NT / 64; ++k)
			t += s_part[k * CNT + tid];
		s_red[tid] = t;
	}
	__syncthreads();
}

} // namespace fh
