// What the block-attention kernels share (block_attention.hip: exact fp32; block_attention16.hip: 16-bit matrix-core
// inputs): the 32-row tile and its accumulator-row map, the workgroup <-> (window, head, row block) map, the argument
// checks and the host-side shape.  One copy, so both forwards cut a batch into workgroups the same way.
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
