// What the 16-bit-input kernels share (half_gemm.hip, edge_gemm16.hip, wgrad16.hip, edge_wgrad16.hip,
// block_attention16.hip): the MFMA of
// each 16-bit type and its fragment maps, the per-wave tile, the rounded LDS panel (row and transposed fragments), the
// rounding store and the transposed read of an LDS image, the fragment epilogue, and the host's dispatch and alignment
// checks.
//
// Operands.  fp32 rows stay fp32 in HBM.  A lane's MFMA A fragment (v_mfma_f32_32x32x16_{bf16,f16}: lane l = row l & 31,
// k = 8 (l >> 5) + j: cdna_hip_programming.md section 3) is 8 consecutive values of its row, rounded to the 16-bit type
// in registers (fptrunc through __builtin_convertvector: round to nearest even, what tensor.to(dtype) does; never a
// truncating pack).  The weights arrive already rounded by the host as 16-bit arrays, so a lane's B fragment (column
// l & 31 of W^T = row l & 31 of W, the same 8 k) is one dwordx4.  Products of two 16-bit values are exact in fp32;
// accumulation and everything after it is fp32.
//
// The chain.  Every kernel here computes an output element as ONE accumulator, zeroed, k ascending in steps of 16 on
// those rounded operands; the two schemes below differ only in where the fragments come from.
//   * wave_tile: a wave owns 32 rows x up to TILES x 32 output columns; a lane rounds its row's fragment straight from
//     the fp32 row (two dwordx4) and reads the weights from L2.  The fragment IS the memory order: no LDS, no barrier.
//     (wave_tile_more continues the same accumulators over a second row: the [x[src] | x[dst]] chain of edge_gemm16.hip.)
//   * RoundedPanel: a workgroup loads ROWS x KT floats ONCE, coalesced (a thread's float4s are consecutive in a row),
//     rounds them and parks them in LDS at a row stride of (KT + 8) x 2 bytes -- an odd number of 16-byte units, so the
//     ds_read_b128 fragment reads of 16 consecutive rows hit 64 distinct banks.  Its waves keep their weights in registers.
//     Two buffers: the next panel's loads are issued before the current panel's MFMAs and land in the other buffer after
//     them, one barrier per panel.
//
// No atomics, no inline assembly; every store is a plain C++ assignment.
#pragma once
#include <type_traits>

#include "dense_common.h"

namespace ptgnn_amd {
namespace half16 {

using f32x4 = __attribute__((ext_vector_type(4))) float;
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

// 4 fp32 values rounded to nearest even into 4 consecutive 16-bit elements (8-byte aligned) of an LDS image
template <int DT>
__device__ __forceinline__ void store4(uint16_t *dst, const float4 &v) {
  using half4 = __attribute__((ext_vector_type(4))) typename Half16<DT>::elem;
  const f32x4 f = {v.x, v.y, v.z, v.w};
  *reinterpret_cast<half4 *>(dst) = __builtin_convertvector(f, half4);
}

// A transposed fragment from two ds_read_b64_tr_b16 (cdna_hip_programming.md T10), through the v4i16 builtin -- bits are
// bits for both 16-bit types, and the files stay free of inline assembly.  Per 16-lane group the instruction gathers a
// 4-row x 16-column block: lane 4 q + p of the group supplies the address of the block's row q, columns 4 p .. 4 p + 3
// (`lo`, and `up` for the second block), and lane i receives column i, rows ascending: lo's in elements 0 .. 3, up's in
// 4 .. 7.  The instruction needs EXEC all ones.
template <int DT>
__device__ __forceinline__ typename Half16<DT>::vec tr8(const uint16_t *lo, const uint16_t *up) {
  using i16x4 = __attribute__((ext_vector_type(4))) short;
  using i16x8 = __attribute__((ext_vector_type(8))) short;
  using lds_i16x4 = __attribute__((address_space(3))) i16x4;
  const i16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)lo);
  const i16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4 *)up);
  return __builtin_bit_cast(typename Half16<DT>::vec, (i16x8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ void zero(f32x16 &acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// this lane in its wave's fragments: row (A), column (B, C) li; k offset 8 hi (A, B), row offset 4 hi (C)
__device__ __forceinline__ int frag_li() { return threadIdx.x & 31; }
__device__ __forceinline__ int frag_hi() { return (threadIdx.x >> 5) & 1; }

// row of C-fragment register r for lane half hi (cdna_hip_programming.md section 3; dtype-independent)
__device__ __forceinline__ int frag_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// The fragment epilogue of a tile whose first row is `row0`: fn(r, row) for each of this lane's 16 C-fragment registers
// r whose row is below `end`.
template <class F>
__device__ __forceinline__ void for_frag_rows(int64_t row0, int64_t end, F &&fn) {
  const int hi = frag_hi();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = row0 + frag_row(r, hi);
    if (row < end) fn(r, row);
  }
}

// The per-edge dropout of the masked forms (edge_gemm16.hip, edge_wgrad16.hip) on one value: v * scale where bit `bit` of
// the keep word is set, else +0 -- the bit spread over the word and ANDed in, as the fp32 streaming kernel does it, so a
// dropped inf or NaN is a zero too.
__device__ __forceinline__ float keep_scaled(float v, uint32_t word, int bit, float scale) {
  const int t = ((int)(word << (31 - bit))) >> 31;
  return __uint_as_float(__float_as_uint(v * scale) & (uint32_t)t);
}
// ... on the 4 consecutive values whose keep bits are bits `bit` .. `bit + 3` of the word
__device__ __forceinline__ float4 keep_scaled4(float4 v, uint32_t word, int bit, float scale) {
  return make_float4(keep_scaled(v.x, word, bit, scale), keep_scaled(v.y, word, bit + 1, scale),
                     keep_scaled(v.z, word, bit + 2, scale), keep_scaled(v.w, word, bit + 3, scale));
}

__device__ __forceinline__ float act_runtime(float v, int act) {
  if (act == PTGNN_AMD_ACT_TANH) return fast_tanh(v);
  if (act == PTGNN_AMD_ACT_RELU) return v > 0.f ? v : 0.f;
  return v;
}

// The per-wave tile: acc[t] = rnd(arow) . rnd(W)[col0 + 32 t + li, :]^T over all of K (K % 32 == 0: two MFMA k-steps
// per trip).  `arow`: the fp32 row of this lane (callers clamp rows past the end onto a valid one; never stored);
// `w`: [*, K] rounded weights; column tiles past `tiles` (>= 1) recompute the last live one.
// wave_tile_more CONTINUES the accumulators over K further columns: `w` then points at those columns of the first weight
// row and `ldw` is the weight rows' stride -- a chain over [a1 | a2] . [W1 | W2]^T is zero, more(a1, W1), more(a2, W2).
template <int DT, int TILES>
__device__ __forceinline__ void wave_tile_more(const float *__restrict__ arow, const uint16_t *__restrict__ w, int ldw,
                                               int K, int col0, int tiles, f32x16 (&acc)[TILES]) {
  using H = Half16<DT>;
  const int li = frag_li(), hi = frag_hi();
  const float *ap = arow + 8 * hi;
  const uint16_t *bp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int tc = t < tiles ? t : tiles - 1;
    bp[t] = w + (int64_t)(col0 + tc * 32 + li) * ldw + 8 * hi;
  }
  for (int kk = 0; kk < K; kk += 32) {
#pragma unroll
    for (int k0 = kk; k0 < kk + 32; k0 += 16) {
      const typename H::vec a = round8<DT>(ap + k0);
#pragma unroll
      for (int t = 0; t < TILES; ++t) acc[t] = H::mfma(a, load8<DT>(bp[t] + k0), acc[t]);
    }
  }
}
template <int DT, int TILES>
__device__ __forceinline__ void wave_tile(const float *__restrict__ arow, const uint16_t *__restrict__ w, int K,
                                          int col0, int tiles, f32x16 (&acc)[TILES]) {
#pragma unroll
  for (int t = 0; t < TILES; ++t) zero(acc[t]);
  wave_tile_more<DT>(arow, w, K, K, col0, tiles, acc);
}

// The rounded panel of a 256-thread workgroup: ROWS x KT values in each of two LDS buffers.  A walk is
//     prime(src of the first panel);
//     per panel: fetch(src of the next panel -- on the last trip its own: no branch around the loads);
//                MFMAs on frag(row, ks); stores; flip();
// where src(r, c) is the address of the 4 floats at row r, columns c .. c + 3 of a panel.
//
// The transposed image (wgrad16.hip: the reduction index of a weight gradient is the panel's ROW index, so a lane's
// fragment is 8 consecutive rows of one column).  Same panel, same park; the row stride LD_ is chosen as 32 x odd
// elements (64 bytes x odd) and the fragments come from frag_tr: two ds_read_b64_tr_b16 (cdna_hip_programming.md T10),
// through the v4i16 builtin -- bits are bits for both 16-bit types, and the file stays free of inline assembly.  Banks
// (section 2 rule: (a / 4) % 64, counted per 32-lane half): a half reads rows q = 0 .. 3 of one 8-row group, 64
// contiguous bytes = 16 banks of each; with a stride of 64 x odd bytes the four rows start at banks {0, 16, 32, 48}
// in some order: 64 distinct banks, no conflict.  (At the row image's stride, KT + 8, the same read would be 4-way.)
// The instruction needs EXEC all ones: rows past the end of the data are ZEROS in the image (`fetch` with `live`),
// never masked lanes, and no caller may `return` or diverge before frag_tr.
template <int DT, int ROWS, int KT, int LD_ = KT + 8>
struct RoundedPanel {
  using vec = typename Half16<DT>::vec;
  using half4 = __attribute__((ext_vector_type(4))) typename Half16<DT>::elem;
  using i16x4 = __attribute__((ext_vector_type(4))) short;
  using i16x8 = __attribute__((ext_vector_type(8))) short;
  static constexpr int LD = LD_;                // LDS row stride in 16-bit elements
  static constexpr int RV = KT / 4;             // float4 per panel row
  static constexpr int NV = ROWS * RV / 256;    // float4 per thread and panel
  static_assert(ROWS * RV % 256 == 0 && LD >= KT && ((LD / 8) % 2 == 1 || LD % 64 == 32), "panel shape");

  float4 stage[NV];
  int cur;

  // the LDS array: static to this instantiation, allocated in every kernel that uses it
  static __device__ __forceinline__ uint16_t *buffer(int buf) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][ROWS * LD];
    return lds[buf];
  }
  template <class Src>
  __device__ __forceinline__ void fetch(Src &&src) {   // a panel's rows -> registers
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      stage[i] = *reinterpret_cast<const float4 *>(src(v / RV, (v % RV) * 4));
    }
  }
  template <class Src>
  __device__ __forceinline__ void fetch(Src &&src, int live) {   // rows >= live: zeros, nothing loaded
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      stage[i] = v / RV < live ? *reinterpret_cast<const float4 *>(src(v / RV, (v % RV) * 4))
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // ... for callers that keep state per staged float4 (edge_wgrad16.hip: the gathered row ids, asked for one panel
  // ahead): src(i, r, c) also gets the slot
  template <class Src>
  __device__ __forceinline__ void fetch_slots(Src &&src, int live) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      stage[i] = v / RV < live ? *reinterpret_cast<const float4 *>(src(i, v / RV, (v % RV) * 4))
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void park(int buf) {      // registers -> rounded 16-bit panel in LDS
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      const f32x4 f = {stage[i].x, stage[i].y, stage[i].z, stage[i].w};
      *reinterpret_cast<half4 *>(buffer(buf) + (v / RV) * LD + (v % RV) * 4) = __builtin_convertvector(f, half4);
    }
  }
  // The hook of the masked forms: fn(i, row, col, value) on each staged float4 (slot i; row, col as `src` got them) of
  // the panel last fetched, before `park` rounds it.  A masked walk is fetch(src); edit(fn); start(); and per panel
  // fetch(next); MFMAs; stores; edit(fn); flip();
  template <class Fn>
  __device__ __forceinline__ void edit(Fn &&fn) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      fn(i, v / RV, (v % RV) * 4, stage[i]);
    }
  }
  __device__ __forceinline__ void start() {            // the fetched panel becomes the current one
    park(0);
    __syncthreads();
    cur = 0;
  }
  template <class Src>
  __device__ __forceinline__ void prime(Src &&src) {
    fetch(src);
    start();
  }
  // this lane's A fragment of k-step ks in row `row` of the current panel
  __device__ __forceinline__ vec frag(int row, int ks) const {
    return *reinterpret_cast<const vec *>(buffer(cur) + row * LD + ks * 16 + 8 * frag_hi());
  }
  template <class Src>
  __device__ __forceinline__ void prime(Src &&src, int live) {
    fetch(src, live);
    start();
  }
  // The transposed fragment: rows row0 + 8 hi .. + 7 (row0 % 8 == 0) of column col0 + li (col0 % 32 == 0) of the
  // current panel, rows ascending in the vector.  Per 16-lane group the instruction gathers a 4-row x 16-column block:
  // lane 4 q + p of the group supplies the address of the block's row q, columns 4 p .. 4 p + 3, and lane i receives
  // column i.  Groups 0, 1 are the two column halves of the rows 8 hi .. (lane half hi = 0), groups 2, 3 of hi = 1.
  __device__ __forceinline__ vec frag_tr(int row0, int col0) const {
    const int l = threadIdx.x & 63, q = (l >> 2) & 3, p = l & 3, g = (l >> 4) & 1;
    const uint16_t *at = buffer(cur) + (row0 + 8 * (l >> 5) + q) * LD + col0 + 16 * g + 4 * p;
    return tr8<DT>(at, at + 4 * LD);
  }
  __device__ __forceinline__ void flip() {
    park(cur ^ 1);
    __syncthreads();                     // the other buffer is complete; everyone is done reading this one
    cur ^= 1;
  }
};

inline bool dtype_ok(int dtype) { return dtype == PTGNN_AMD_HALF_BF16 || dtype == PTGNN_AMD_HALF_F16; }

// a float matrix the fragment loads can read: 16-byte aligned base, rows a multiple of 16 bytes apart
inline bool rows16(const void *p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// Host dispatch of a runtime value onto template arguments: calls fn(std::integral_constant<int, V>) for the V among
// Vs that equals v.  False: none does.
template <int... Vs, class F>
bool with_case(int v, F &&fn) {
  return ((v == Vs ? (fn(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
bool with_dtype(int dtype, F &&fn) {
  return with_case<PTGNN_AMD_HALF_BF16, PTGNN_AMD_HALF_F16>(dtype, fn);
}

}  // namespace half16
}  // namespace ptgnn_amd
