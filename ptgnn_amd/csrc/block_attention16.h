// What the 16-bit-input block-attention kernels share (block_attention16.hip: the forward, with and without dropout;
// block_attention16_backward.hip: the two gradient kernels): the workgroup size, the two LDS row strides of a rounded
// [row][d] image and the fp32 row load of the staging.
//
// LDS images.  A tile that is the A or B operand of a product over d is read by rows (one ds_read_b128 per lane and
// k-step): its row stride is d padded to 16, + 8 elements -- an odd number of 16-byte units (half16.h).  A tile whose
// ROW index is summed (the second products: the probabilities or score gradients come from the accumulator registers
// and the tile is the B operand) is read transposed (ds_read_b64_tr_b16): its row stride is 32 x odd elements, so the
// four rows of a half's read start 16 banks apart.  The two patterns have no common conflict-free stride (the row read
// wants 16 bytes x odd, the transposed one 64 bytes x odd: at either stride the other read is 4-way conflicted), so a
// tile that is read both ways is parked as TWO images, one per stride.
#pragma once
#include "block_attention.h"
#include "half16.h"

namespace ptgnn_amd {

constexpr int kBa16Threads = 64 * kBaMaxWaves;
constexpr int kBa16Rows = kBaTile * kBaMaxWaves;   // the rows a workgroup owns

// LDS row strides in 16-bit elements: row reads (d = dk or dv), transposed reads (dt = 32-column tiles)
inline int ba16_ldk(int d) { return (d + 15) / 16 * 16 + 8; }
constexpr int ba16_ldv(int dt) { return 32 * (dt | 1); }

// columns c .. c + 3 of a row of `width` live columns (c % 4 == 0; columns past the width: 0).  `vec`: the row is 16-byte
// aligned and width % 4 == 0, so a live c has all four
__device__ __forceinline__ float4 ba16_load4(const float *__restrict__ row, int c, int width, bool vec) {
  if (vec) return c < width ? *reinterpret_cast<const float4 *>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = c < width ? row[c] : 0.f;
  v.y = c + 1 < width ? row[c + 1] : 0.f;
  v.z = c + 2 < width ? row[c + 2] : 0.f;
  v.w = c + 3 < width ? row[c + 3] : 0.f;
  return v;
}

// this lane's address offset inside a 4-row x 16-column block of a transposed read at row stride `ld` (half16.h, tr8):
// rows 4 h + q of the block's 8-row group, column half g, columns 4 p ..
__device__ __forceinline__ int ba16_tr_off(int lane, int ld) {
  return (4 * (lane >> 5) + ((lane >> 2) & 3)) * ld + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
}

// registers 8 s .. 8 s + 7 of an accumulator tile, rounded once: the A operand of k-step s of the next product (the
// summed index runs over the tile rows ba_row(8 s + i, h), which is what the two transposed reads of that step fetch)
template <int DT>
__device__ __forceinline__ typename half16::Half16<DT>::vec ba16_round8(const f32x16 &x, int s) {
  const half16::f32x8 f = {x[8 * s], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3],
                           x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]};
  return __builtin_convertvector(f, typename half16::Half16<DT>::vec);
}

// acc = sum_d A[lane row][d] B[lane row][d] over `steps` k-steps of two row images (addresses of this lane's 8 values of
// step 0)
template <int DT>
__device__ __forceinline__ f32x16 ba16_nt(const uint16_t *a, const uint16_t *b, int steps) {
  f32x16 x;
  half16::zero(x);
  for (int s = 0; s < steps; ++s)
    x = half16::Half16<DT>::mfma(half16::load8<DT>(a + 16 * s), half16::load8<DT>(b + 16 * s), x);
  return x;
}

// z[t] += sum_i rnd(x[8 s + i]) tile[ba_row(8 s + i, h)][32 t + lane column], s = 0, 1: `tile` is this lane's address in
// the transposed image (ba16_tr_off already added), row stride LDT
template <int DT, int T, int LDT>
__device__ __forceinline__ void ba16_tn(f32x16 (&z)[T], const f32x16 &x, const uint16_t *tile) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const typename half16::Half16<DT>::vec a = ba16_round8<DT>(x, s);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint16_t *at = tile + 16 * s * LDT + 32 * t;
      z[t] = half16::Half16<DT>::mfma(a, half16::tr8<DT>(at, at + 8 * LDT), z[t]);
    }
  }
}

}  // namespace ptgnn_amd
