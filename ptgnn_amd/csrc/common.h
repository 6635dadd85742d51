// Shared helpers for libptgnn_amd (gfx950 only; no portability layer by design).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ptgnn_amd.h"

namespace ptgnn_amd {

void set_error(const char *fmt, ...);
void count_launch(int kernel_id);   // PTGNN_AMD_KERNEL_* of include/ptgnn_amd.h

#define PTGNN_REQUIRE(cond, code, ...)            \
  do {                                            \
    if (!(cond)) {                                \
      ::ptgnn_amd::set_error(__VA_ARGS__);        \
      return (code);                              \
    }                                             \
  } while (0)

#define PTGNN_HIP(expr)                                                                    \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      ::ptgnn_amd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                             __FILE__, __LINE__);                                          \
      return PTGNN_AMD_EHIP;                                                               \
    }                                                                                      \
  } while (0)

#define PTGNN_LAUNCH_CHECK()                                                               \
  do {                                                                                     \
    hipError_t _e = hipGetLastError();                                                     \
    if (_e != hipSuccess) {                                                                \
      ::ptgnn_amd::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),    \
                             __FILE__, __LINE__);                                          \
      return PTGNN_AMD_EHIP;                                                               \
    }                                                                                      \
  } while (0)

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kNumXcd = 8;       // MI355X: 8 XCDs, block b is observed on XCD b % 8

// XCD-aware tile order: consecutive tiles go to the SAME XCD (contiguous node ranges -- i.e. whole
// graphs of a disjoint-union batch -- share one 4 MiB L2), while hardware round-robins blockIdx
// over the XCDs.  Performance only; correctness never depends on placement.
__device__ __forceinline__ int64_t xcd_swizzle(int64_t block, int64_t nblocks) {
  const int64_t per = (nblocks + kNumXcd - 1) / kNumXcd;
  const int64_t tile = (block % kNumXcd) * per + block / kNumXcd;
  return tile;  // may be >= nblocks for the ragged tail: caller must bounds-check
}

inline int64_t xcd_padded_blocks(int64_t nblocks) {
  const int64_t per = (nblocks + kNumXcd - 1) / kNumXcd;
  return per * kNumXcd;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Raise a kernel's dynamic-LDS limit to `bytes`, once per (kernel, device): the attribute call is not legal while a
// stream is being captured into a hipGraph, and the warm-up launch outside the capture has made the call, so a launch
// inside a capture finds the limit cached.  false when the runtime refuses (the caller decides what that means; `why`
// then receives the runtime's error string).
bool raise_dynamic_lds(const void *fn, size_t bytes, const char **why = nullptr);   // errors.cpp
template <typename Kern>
bool raise_dynamic_lds(Kern kern, size_t bytes, const char **why = nullptr) {
  return raise_dynamic_lds(reinterpret_cast<const void *>(kern), bytes, why);
}

#ifdef __HIPCC__
// Row math with a bitwise contract between its users: the fused inference epilogue (gather_reduce_core.h) and the training
// pair (row_epilogue.hip) must round alike, so there is one copy.
__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

__device__ __forceinline__ float gelu_erf_grad(float x) {
  // d/dx [x Phi(x)] = Phi(x) + x phi(x)
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

// VEC (4 or 1) consecutive floats of a row as one float4 or one float access
template <int VEC>
__device__ __forceinline__ void vec_load(const float *p, float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  } else {
    o[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void vec_store(float *p, const float (&o)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
  else *p = o[0];
}
#endif

}  // namespace ptgnn_amd
