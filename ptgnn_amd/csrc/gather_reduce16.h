// What the two aggregations over 16-bit message rows share (gather_reduce16.hip: the plain fold of the GGNN layer;
// gather_reduce16_epi.hip: the MLP-MP layer's fold with a destination term and a GELU / LayerNorm finish): the 16-byte
// vector a lane loads, the up-cast of a 16-bit pair, and the shapes both take.
#pragma once
#include "common.h"

namespace ptgnn_amd {
namespace {

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// the two 16-bit values of a dword as fp32: element 0 is the low half
template <int DT>
__device__ __forceinline__ void widen2(uint32_t w, float &lo, float &hi) {
  if constexpr (DT == PTGNN_AMD_HALF_BF16) {
    lo = __uint_as_float(w << 16);
    hi = __uint_as_float(w & 0xffff0000u);
  } else {
    const f32x2 f = __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2);
    lo = f[0];
    hi = f[1];
  }
}

inline bool shape_ok16(int32_t msg_dim) { return msg_dim > 0 && msg_dim % 32 == 0 && msg_dim <= 256; }
inline bool dtype_ok16(int dtype) { return dtype == PTGNN_AMD_HALF_BF16 || dtype == PTGNN_AMD_HALF_F16; }

}  // namespace
}  // namespace ptgnn_amd
