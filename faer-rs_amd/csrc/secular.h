// Scalar helpers, wavefront / workgroup reductions, Givens rotations and the secular equation root finder of the divide
// and conquer solvers (evd.hip: symmetric tridiagonal, svd.hip: bidiagonal; dnc.h has the driver scaffolding they share).
// secular_root is the reference's secular_eq_root_finder (svd/bidiag_svd.rs:7-270), which both of its solvers call.
#pragma once
#include <cmath>

#include "common.h"

namespace fh {

namespace {

template <typename T> struct DncTraits;
template <> struct DncTraits<double> {
	static constexpr double eps = 2.220446049250313e-16;
	static constexpr double sml = 2.2250738585072014e-308;
	static constexpr long iter_factor = 32; // max(30, nbits / 2)
};
template <> struct DncTraits<float> {
	static constexpr float eps = 1.1920929e-07f;
	static constexpr float sml = 1.17549435e-38f;
	static constexpr long iter_factor = 30;
};

__device__ __forceinline__ double ev_abs(double x) { return fabs(x); }
__device__ __forceinline__ float ev_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double ev_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float ev_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double ev_hypot(double x, double y) { return hypot(x, y); }
__device__ __forceinline__ float ev_hypot(float x, float y) { return hypotf(x, y); }
template <typename T> __device__ __forceinline__ T ev_max(T a, T b) { return a > b ? a : b; } // fmax of two non-NaN values
template <typename T> __device__ __forceinline__ T ev_inf() { return (T) INFINITY; }

template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o);
	return __shfl(v, 0); // every lane takes lane 0's sum: the callers branch on it, so all lanes must see the same bits
}
template <typename T> __device__ __forceinline__ T wave_max(T v)
{
	for (int o = 32; o > 0; o >>= 1)
		v = ev_max(v, __shfl_xor(v, o));
	return v;
}
// 256-thread blocks: sum / max of one value per thread, the result in every thread
template <typename T, bool MAX> __device__ T block_reduce(T v, T *red)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	v = MAX ? wave_max(v) : wave_sum(v);
	__syncthreads(); // red may still be read by the previous reduction
	if (lane == 0)
		red[w] = v;
	__syncthreads();
	T r = red[0];
	for (int i = 1; i < 4; ++i)
		r = MAX ? ev_max(r, red[i]) : r + red[i];
	return r;
}

template <typename T> __device__ __forceinline__ void make_givens(T p, T q, T &c, T &s)
{
	// linalg/jacobi.rs:16-55
	if (q == (T) 0) {
		c = p < (T) 0 ? (T) -1 : (T) 1;
		s = 0;
	} else if (p == (T) 0) {
		c = 0;
		s = q < (T) 0 ? (T) 1 : (T) -1;
	} else if (ev_abs(p) > ev_abs(q)) {
		const T t = q / p;
		T u = ev_hypot(t, (T) 1);
		if (p < (T) 0)
			u = -u;
		c = (T) 1 / u;
		s = -t * c;
	} else {
		const T t = p / q;
		T u = ev_hypot(t, (T) 1);
		if (q < (T) 0)
			u = -u;
		s = -(T) 1 / u;
		c = -t * s;
	}
}

// secular_eq_root_finder (svd/bidiag_svd.rs:7-270) evaluated by a whole wavefront; every lane holds the same scalars
template <typename T> struct SecularEq {
	const T *d, *z;
	int k;
	T rho_recip;
	__device__ T operator()(T shift, T mu) const
	{
		T acc = 0;
		for (int i = (int) (threadIdx.x & 63); i < k; i += 64) {
			const T zi = z[i];
			acc += zi * (zi / ((d[i] - shift) - mu));
		}
		return rho_recip + wave_sum(acc);
	}
};

template <typename T, typename F> __device__ void secular_root(const F &f, T left, T right, bool last, T &shift_out, T &mu_out)
{
	const T two = 2, eight = 8, one_half = 0.5, epsilon = DncTraits<T>::eps;
	// loop caps: none is reached by a convergent search, they only keep a non-finite input from spinning
	constexpr int SECANT_CAP = 256, BISECT_CAP = 2200;
	const T mid = left + (right - left) * one_half;
	T f_mid = f((T) 0, mid);
	const T f_max = f(left, last ? right - left : (right - left) * one_half);
	const T f_mid_left_shift = f(left, (right - left) * one_half);
	const T f_mid_right_shift = f(right, (left - right) * one_half);
	T shift, mu;
	if (last || f_mid > (T) 0) {
		shift = left;
		mu = (right - left) * one_half;
	} else {
		shift = right;
		mu = (left - right) * one_half;
	}
	if (f_mid_left_shift <= (T) 0 && f_mid_right_shift > (T) 0) {
		shift_out = shift;
		mu_out = mu;
		return;
	}
	if (!last) {
		if (shift == left) {
			if (f_mid_left_shift < (T) 0) {
				shift = right;
				f_mid = f_mid_right_shift;
			}
		} else if (f_mid_right_shift > (T) 0) {
			shift = left;
			f_mid = f_mid_left_shift;
		}
	}
	T left_shifted, f_left, right_shifted, f_right;
	if (shift == left) {
		left_shifted = 0;
		f_left = -ev_inf<T>();
		right_shifted = last ? right - left : (right - left) * one_half;
		f_right = last ? f_max : f_mid;
	} else {
		left_shifted = (left - right) * one_half;
		f_left = f_mid;
		right_shifted = 0;
		f_right = ev_inf<T>();
	}
	int iteration_count = 0;
	T f_prev = f_mid;
	const T half0 = one_half, half1 = half0 * half0, half2 = half1 * half1, half3 = half2 * half2;
	const T base = shift == left ? right_shifted : left_shifted;
	const T mu_values[4] = {base * half3, base * half2, base * half1, base * half0};
	T f_values[4];
	for (int t = 0; t < 4; ++t)
		f_values[t] = f(shift, mu_values[t]);
	if (shift == left) {
		int i = 0;
		for (int t = 0; t < 4; ++t)
			if (f_values[t] < (T) 0) {
				left_shifted = mu_values[t];
				f_left = f_values[t];
				i = t + 1;
			}
		if (i < 4) {
			right_shifted = mu_values[i];
			f_right = f_values[i];
		}
	} else {
		int i = 0;
		for (int t = 0; t < 4; ++t)
			if (f_values[t] > (T) 0) {
				right_shifted = mu_values[t];
				f_right = f_values[t];
				i = t + 1;
			}
		if (i < 4) {
			left_shifted = mu_values[i];
			f_left = f_values[i];
		}
	}
	while (right_shifted - left_shifted > two * epsilon * ev_max(ev_abs(left_shifted), ev_abs(right_shifted))) {
		const T mid_a = (left_shifted + right_shifted) * one_half;
		T mid_g = ev_sqrt(ev_abs(left_shifted)) * ev_sqrt(ev_abs(right_shifted));
		if (left_shifted < (T) 0)
			mid_g = -mid_g;
		const T mid_shifted = mid_g == (T) 0 ? mid_a : mid_g;
		const T fm = f(shift, mid_shifted);
		if (fm == (T) 0) {
			shift_out = shift;
			mu_out = mid_shifted;
			return;
		} else if (fm > (T) 0) {
			right_shifted = mid_shifted;
			f_prev = f_right;
			f_right = fm;
		} else {
			left_shifted = mid_shifted;
			f_prev = f_left;
			f_left = fm;
		}
		if (iteration_count == 4)
			break;
		++iteration_count;
	}
	T mu_cur, mu_prev, f_cur, f_prv;
	if (left_shifted == (T) 0) {
		mu_cur = right_shifted * two;
		mu_prev = right_shifted;
		f_cur = f_prev;
		f_prv = f_right;
	} else if (right_shifted == (T) 0) {
		mu_cur = left_shifted * two;
		mu_prev = left_shifted;
		f_cur = f_prev;
		f_prv = f_left;
	} else {
		mu_cur = left_shifted;
		mu_prev = right_shifted;
		f_cur = f_left;
		f_prv = f_right;
	}
	// secant (bidiag_svd.rs:56-126)
	if (ev_abs(f_prv) < ev_abs(f_cur)) {
		T t = f_prv;
		f_prv = f_cur;
		f_cur = t;
		t = mu_prev;
		mu_prev = mu_cur;
		mu_cur = t;
	}
	bool has_l = false, has_r = false, use_bisection = false;
	T lc = 0, rcand = 0;
	if ((f_prv > (T) 0) != (f_cur > (T) 0)) {
		lc = mu_cur < mu_prev ? mu_cur : mu_prev;
		rcand = mu_cur < mu_prev ? mu_prev : mu_cur;
		has_l = has_r = true;
	}
	for (int it = 0; it < SECANT_CAP && f_cur != (T) 0 &&
			 ev_abs(mu_cur - mu_prev) > eight * epsilon * ev_max(ev_abs(mu_cur), ev_abs(mu_prev)) && ev_abs(f_cur - f_prv) > epsilon &&
			 !use_bisection;
	     ++it) {
		const T a = (f_cur - f_prv) * (mu_prev * mu_cur) / (mu_prev - mu_cur);
		const T bb = f_cur - a / mu_cur;
		const T mu_zero = -a / bb;
		const T f_zero = f(shift, mu_zero);
		if (f_zero < (T) 0) {
			lc = mu_zero;
			has_l = true;
		} else {
			rcand = mu_zero;
			has_r = true;
		}
		mu_prev = mu_cur;
		f_prv = f_cur;
		mu_cur = mu_zero;
		f_cur = f_zero;
		if (shift == left && (mu_cur < (T) 0 || mu_cur > right - left))
			use_bisection = true;
		if (shift == right && (mu_cur > (T) 0 || mu_cur < left - right))
			use_bisection = true;
		if (ev_abs(f_cur) > ev_abs(f_prv)) {
			T kk = 1;
			for (int t = 0; t < 4; ++t) {
				const T mu_opp = -a / (kk * f_zero + bb);
				const T f_opp = f(shift, mu_opp);
				if (f_zero < (T) 0 && f_opp >= (T) 0) {
					rcand = mu_opp;
					has_r = true;
					break;
				}
				if (f_zero > (T) 0 && f_opp <= (T) 0) {
					lc = mu_opp;
					has_l = true;
					break;
				}
				kk = kk * two;
			}
			use_bisection = true;
		}
	}
	if (has_l && has_r && lc < rcand) {
		if (lc > left_shifted)
			left_shifted = lc;
		if (rcand < right_shifted)
			right_shifted = rcand;
	}
	if (use_bisection) {
		for (int it = 0; it < BISECT_CAP && right_shifted - left_shifted > two * epsilon * ev_max(ev_abs(left_shifted), ev_abs(right_shifted));
		     ++it) {
			const T mid_shifted = (left_shifted + right_shifted) * one_half;
			const T fm = f(shift, mid_shifted);
			if (fm == (T) 0)
				break;
			else if (fm > (T) 0)
				right_shifted = mid_shifted;
			else
				left_shifted = mid_shifted;
		}
		mu_cur = (left_shifted + right_shifted) * one_half;
	}
	shift_out = shift;
	mu_out = mu_cur;
}

} // namespace

} // namespace fh
