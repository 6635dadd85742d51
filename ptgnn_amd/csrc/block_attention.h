// What the block-attention kernels share (block_attention.hip: exact fp32; block_attention16.hip and
// block_attention16_backward.hip: 16-bit matrix-core inputs): the 32-row tile and its accumulator-row map, the workgroup
// <-> (window, head, row block) map, the dropout multiplier of a probability, the row-dot kernel of the backwards, the
// argument checks and the host-side shape.  One copy, so every kernel cuts a batch into workgroups the same way and the
// same seed drops the same probabilities on both routes.
#pragma once
#include "dense_common.h"

namespace ptgnn_amd {

constexpr int kBaTile = 32;          // rows of one MFMA tile: a wave's rows, and the rows of a staged tile
constexpr int kBaMaxWaves = 4;       // waves (32-row tiles) of a workgroup
constexpr int kBaMaxDim = 128;
constexpr float kLog2e = 1.4426950408889634f;

struct BaShape {
  int heads, dk, dv, dkt, dvt, row_tiles;   // dkt / dvt: 32-column tiles of dk / dv
  float scale;
};

// row of register r of a 32x32 accumulator tile in lane half h
__device__ __forceinline__ int ba_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float ba_exp(float v) { return __builtin_amdgcn_exp2f(v * kLog2e); }

// The dropout multiplier (scale or 0) of the probability of (mask row, window column j): the stateless hash of
// dense_common.h on a [N heads, W] mask, W = max_num_nodes rounded up to even (ba_dropout), mask row = r heads + h.
__device__ __forceinline__ float ba_keep(const DropoutParams &d, int64_t row, int j) {
  const uint32_t b = dropout_bits(d, row, j >> 1);
  return ((j & 1) ? (b >> 16) : (b & 0xffffu)) >= d.thr ? d.scale : 0.0f;
}

inline DropoutParams ba_dropout(float p, uint64_t seed, int32_t max_nodes) {
  return make_dropout(p, seed, (max_nodes + 1) / 2 * 2);
}

// D[r, head] = sum_d grad_out[r, head dv + d] out[r, head dv + d], d ascending (fp32, unrounded operands)
static __global__ __launch_bounds__(256) void k_block_attention_rowdot(const float *__restrict__ go, int64_t ld_go,
                                                                       const float *__restrict__ out, int64_t ld_out,
                                                                       int64_t num_rows, int heads, int dv,
                                                                       float *__restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_rows * heads) return;
  const int64_t r = i / heads;
  const int head = (int)(i % heads);
  const float *a = go + r * ld_go + (int64_t)head * dv, *b = out + r * ld_out + (int64_t)head * dv;
  float t = 0.0f;
  for (int d = 0; d < dv; ++d) t = fmaf(a[d], b[d], t);
  D[i] = t;
}

// The staging and the two exact-fp32 MFMA products of block_attention.hip's header comment ("NT", "TN"), shared with
// projection_loss.hip, whose score tiles are the same algebra over (decoding locations, vocabulary entries).
// dst[r][c] (row stride ldd) = src[min(row0 + r, row_end - 1)][c] for c < width, 0 for width <= c < widthp
__device__ __forceinline__ void ba_stage(float *__restrict__ dst, int ldd, const float *__restrict__ src, int64_t ld,
                                         int row0, int row_end, int rows, int width, int widthp) {
  const int step = blockDim.x >> 5;
  for (int r = threadIdx.x >> 5; r < rows; r += step) {
    int64_t g = (int64_t)row0 + r;
    if (g >= row_end) g = row_end - 1;
    const float *p = src + g * ld;
    for (int c = threadIdx.x & 31; c < widthp; c += 32) dst[r * ldd + c] = c < width ? p[c] : 0.0f;
  }
}

// C[i, j] = sum_d A[i, d] B[j, d]
__device__ __forceinline__ f32x16 ba_nt(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                        int ksteps, int lane) {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.0f;
  const float *a = A + (lane & 31) * lda + (lane >> 5);
  const float *b = B + (lane & 31) * ldb + (lane >> 5);
  for (int s = 0; s < ksteps; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], b[2 * s], c, 0, 0, 0);
  return c;
}

// Z_t[i, j] += sum_r X[r, i] B[r, 32 t + j], t < T
template <int T>
__device__ __forceinline__ void ba_tn(f32x16 (&z)[T], const f32x16 &x, const float *__restrict__ B, int ldb, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float *b = B + ba_row(s, h) * ldb + (lane & 31);
#pragma unroll
    for (int t = 0; t < T; ++t) z[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s], b[32 * t], z[t], 0, 0, 0);
  }
}

// workgroup -> its window [start, end) and first row r0 inside it; false when it has no rows
__device__ __forceinline__ bool ba_locate(const int32_t *__restrict__ windows, const BaShape &sh, int &start, int &end,
                                          int &r0) {
  const int w = blockIdx.x / sh.row_tiles, rt = blockIdx.x % sh.row_tiles;
  start = windows[w];
  end = windows[w + 1];
  r0 = rt * kBaTile * (int)(blockDim.x >> 6);
  return r0 < end - start;
}

// a workgroup beyond 64 KiB of LDS needs the kernel's limit raised first
template <typename Kern>
bool ba_lds_ok(Kern kern, size_t bytes) { return bytes <= 64 * 1024 || raise_dynamic_lds(kern, bytes); }

// the checks the forwards and the backward share; 0 when the arguments are fine
inline int ba_check(const char *what, const void *kqv, int64_t ld, const void *windows, int64_t num_windows,
                    int64_t num_rows, int32_t max_nodes, int32_t heads, int32_t dk, int32_t dv, float p) {
  PTGNN_REQUIRE(num_windows >= 0 && num_rows >= 0 && max_nodes > 0 && heads > 0 && dk > 0 && dv > 0, PTGNN_AMD_EINVAL,
                "%s: bad sizes", what);
  PTGNN_REQUIRE(dk <= kBaMaxDim && dv <= kBaMaxDim, PTGNN_AMD_EUNSUPPORTED,
                "%s: key / value dimension (%d, %d) exceeds %d", what, dk, dv, kBaMaxDim);
  PTGNN_REQUIRE(p >= 0.0f && p < 1.0f, PTGNN_AMD_EINVAL, "%s: dropout rate %g outside [0, 1)", what, (double)p);
  PTGNN_REQUIRE(heads <= 65535, PTGNN_AMD_EUNSUPPORTED, "%s: more than 65535 heads", what);
  if (num_rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(kqv && windows, PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE(num_windows > 0, PTGNN_AMD_EINVAL, "%s: rows without windows", what);
  PTGNN_REQUIRE(ld >= (int64_t)heads * (2 * dk + dv), PTGNN_AMD_EINVAL, "%s: bad leading dimension", what);
  PTGNN_REQUIRE(num_rows * heads < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many rows", what);
  return PTGNN_AMD_OK;
}

inline BaShape ba_shape(int32_t heads, int32_t dk, int32_t dv, int nw, int64_t num_rows, int32_t max_nodes) {
  BaShape sh;
  sh.heads = heads;
  sh.dk = dk;
  sh.dv = dv;
  sh.dkt = (dk + 31) / 32;
  sh.dvt = (dv + 31) / 32;
  const int64_t longest = num_rows < max_nodes ? num_rows : max_nodes;      // no window is longer
  sh.row_tiles = (int)((longest + kBaTile * nw - 1) / (kBaTile * nw));
  sh.scale = (float)(1.0 / sqrt((double)dk));
  return sh;
}

#define BA_TILES(n, ...)          \
  switch (n) {                    \
    case 1: { constexpr int TT = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int TT = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int TT = 3; __VA_ARGS__; } break; \
    default: { constexpr int TT = 4; __VA_ARGS__; } break; \
  }

}  // namespace ptgnn_amd
