// The wave-level building blocks of the kernels (device code only): the xor shuffle of a value, the butterfly sum / max
// of a scalar over a lane group, the inclusive scan of a wave, the butterfly fold of a struct, and "lane 0 of every wave
// to LDS, one barrier, the waves folded in wave order".  The promises the kernels make -- no float atomics, every lane
// ends with the same bits, folded in wave order -- rest on the orders spelled here, once:
//   butterfly   offsets LANES / 2, ..., 1 at shuffle width LANES.  With a commutative step every lane of the group ends
//               with the same bits.
//   wave order  lds[0] folded with lds[1], ..., lds[WAVES - 1], in that order.
// Workgroups are one-dimensional: lane = threadIdx.x & 63, wave = threadIdx.x >> 6.
#pragma once
#include <type_traits>

#include "common.h"

namespace ptgnn_amd {

// v of lane (l ^ o) inside the aligned group of `width` lanes; 64-bit values travel as two dwords
__device__ __forceinline__ float lane_xor(float v, int o, int width = kWave) { return __shfl_xor(v, o, width); }
__device__ __forceinline__ int lane_xor(int v, int o, int width = kWave) { return __shfl_xor(v, o, width); }
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int o, int width = kWave) { return __shfl_xor(v, o, width); }

__device__ __forceinline__ int64_t lane_xor(int64_t v, int o, int width = kWave) {
  const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, o, width);
  const int hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), o, width);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ double lane_xor(double v, int o, int width = kWave) {
  return __longlong_as_double(lane_xor((int64_t)__double_as_longlong(v), o, width));
}

// sum / maximum of `v` over the LANES consecutive lanes of a group: every lane ends with the same bits
template <int LANES = kWave, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v += lane_xor(v, o, LANES);
  return v;
}

template <int LANES = kWave, typename T>
__device__ __forceinline__ T group_max(T v) {
  static_assert(std::is_same_v<T, float> || std::is_same_v<T, int>, "group_max: float (fmaxf) and int only");
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) {
    const T other = lane_xor(v, o, LANES);
    if constexpr (std::is_same_v<T, float>) v = fmaxf(v, other);
    else v = other > v ? other : v;
  }
  return v;
}

// group_sum for a lane count known only at run time (a power of two <= 64; the shuffles are 64 wide): the one run-time form
__device__ __forceinline__ float lanes_sum(float v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += lane_xor(v, o);
  return v;
}

// lane l gets the sum of `v` over the lanes 0 .. l of its wave.  The wave-level ladder only: what a kernel does across
// its waves, and with which barriers, stays with the kernel.
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// An order as the merge of a fold: first_by(before)(a, b) keeps `a` unless before(b, a), "the newcomer comes first".
template <typename Before>
struct FirstBy {
  Before before;
  template <typename T>
  __device__ __forceinline__ T operator()(T a, const T &b) const {
    if (before(b, a)) a = b;
    return a;
  }
};

template <typename Before>
__device__ __forceinline__ FirstBy<Before> first_by(Before before) { return FirstBy<Before>{before}; }

// the butterfly over a struct with the merge T f(a, b): T needs a lane_xor(const T &, int) of its own
template <typename T, typename F>
__device__ __forceinline__ T wave_fold(T a, F f) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) a = f(a, lane_xor(a, o));
  return a;
}

// The two halves of waves_in_order, for a kernel that puts several values behind ONE barrier.
template <typename T>
__device__ __forceinline__ void leader_store(const T &a, T *lds) {
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = a;
}

template <int WAVES, typename T, typename F>
__device__ __forceinline__ T fold_in_order(const T *lds, F f) {
  T a = lds[0];
  for (int w = 1; w < WAVES; ++w) a = f(a, lds[w]);
  return a;
}

// Lane 0 of every wave stores its value, ONE __syncthreads(), then the WAVES values are folded in wave order by every
// thread -- or, with `folds` false, not by this one, which gets `a` back (a kernel where only thread 0 needs the result
// passes threadIdx.x == 0).  A caller that writes `lds` again puts its own barrier behind the call.
template <int WAVES, typename T, typename F>
__device__ __forceinline__ T waves_in_order(T a, T *lds, F f, bool folds = true) {
  leader_store(a, lds);
  __syncthreads();
  return folds ? fold_in_order<WAVES>(lds, f) : a;
}

}  // namespace ptgnn_amd
