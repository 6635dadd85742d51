// What the 16-bit-input kernels share (half_gemm.hip, edge_gemm16.hip): the MFMA of each 16-bit type, the rounding
// fragment load, the pre-rounded weight load and the C-fragment row map (cdna_hip_programming.md section 3).
#pragma once
#include "dense_common.h"

namespace ptgnn_amd {
namespace half16 {

using f32x8 = __attribute__((ext_vector_type(8))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

template <int DT>
struct Half16;
template <>
struct Half16<PTGNN_AMD_HALF_BF16> {
  using vec = bf16x8;
  using elem = __bf16;
  static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Half16<PTGNN_AMD_HALF_F16> {
  using vec = f16x8;
  using elem = _Float16;
  static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// 8 consecutive fp32 values (32-byte aligned) rounded to nearest even into one MFMA fragment
template <int DT>
__device__ __forceinline__ typename Half16<DT>::vec round8(const float *__restrict__ p) {
  const float4 lo = *reinterpret_cast<const float4 *>(p), hi = *reinterpret_cast<const float4 *>(p + 4);
  const f32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return __builtin_convertvector(v, typename Half16<DT>::vec);
}

// 8 consecutive 16-bit weights (16-byte aligned), already rounded by the host
template <int DT>
__device__ __forceinline__ typename Half16<DT>::vec load8(const uint16_t *__restrict__ p) {
  return *reinterpret_cast<const typename Half16<DT>::vec *>(p);
}

__device__ __forceinline__ void zero(f32x16 &acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// row of C-fragment register r for lane half hi (cdna_hip_programming.md section 3; dtype-independent)
__device__ __forceinline__ int frag_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

__device__ __forceinline__ float act_runtime(float v, int act) {
  if (act == PTGNN_AMD_ACT_TANH) return fast_tanh(v);
  if (act == PTGNN_AMD_ACT_RELU) return v > 0.f ? v : 0.f;
  return v;
}

inline bool dtype_ok(int dtype) { return dtype == PTGNN_AMD_HALF_BF16 || dtype == PTGNN_AMD_HALF_F16; }

}  // namespace half16
}  // namespace ptgnn_amd
