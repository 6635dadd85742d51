// The row tile of the segment kernels that dot every row of a chunk with a few per-segment vectors: attention_pool.hip
// (heads of u, and of dP in its backward) and segment_scores.hip (the L decoder states of a sample).  One copy of the
// staging of the vectors and of the rows into LDS and of the score walk, so the two kernels
// read a tile the same way; and the one launch helper that opts a kernel into more than 64 KiB of LDS.
//
// A tile is R rows of a chunk (segment_chunks.h) staged as xs[r * S + :] with S = dim | 1 (odd: lanes reading 32 rows at
// one column hit 32 banks); the vectors lie in LDS as [dim][HP] (HP = vectors padded to a float4, the padding 0) and are
// read as broadcast float4.  Thread (row r, part p) of the score walk dots ITS column slice of x_r with every vector; a
// half-wave then adds the parts of a row in a fixed order (group_sum<32> / group_max<32> of wave_ops.h).
#pragma once
#include "wave_ops.h"

namespace ptgnn_amd {

// Limits of the tile, not of one kernel: attention_pool.hip takes kAttnMaxHeads as its head limit and segment_scores.hip
// as its limit on the vectors of a sample (one half-wave of the 256 threads per vector), and both size their LDS from
// these.  Raising one changes the supported range of both kernels.
constexpr int kAttnThreads = 256;
constexpr int kAttnMaxHeads = 8;
constexpr int kAttnMaxDim = 1024;
constexpr size_t kAttnMaxLds = 160 * 1024;     // LDS of one CU (gfx950)

#ifdef __HIPCC__
// [dim][HP] image of the segment's [heads][dim] rows (padded heads 0)
template <int HP>
__device__ __forceinline__ void attn_stage_heads(float *__restrict__ dst, const float *__restrict__ src, int dim,
                                                 int heads) {
  for (int e = threadIdx.x; e < dim * HP; e += kAttnThreads) {
    const int d = e / HP, h = e % HP;
    dst[e] = h < heads ? src[(int64_t)h * dim + d] : 0.0f;
  }
}

// the tile's rows x[perm[t0 + r], :] -> xs[r * S + :]
__device__ __forceinline__ void attn_stage_rows(float *__restrict__ xs, int S, const float *__restrict__ x, int64_t ld_x,
                                                const int32_t *__restrict__ perm, int t0, int rows, int dim, bool vec4) {
  if (vec4) {
    // batches of kStageBatch loads in flight per thread before their LDS stores: one memory round trip per batch
    // (a tile of 32 rows x 256 columns is 8 float4 per thread)
    constexpr int kStageBatch = 8;
    const int d4 = dim >> 2, total = rows * d4;
    for (int base = threadIdx.x; base < total; base += kStageBatch * kAttnThreads) {
      float4 v[kStageBatch];
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) {
        const int e = base + k * kAttnThreads;
        if (e < total) {
          const int r = e / d4, c = (e - r * d4) << 2;
          v[k] = *reinterpret_cast<const float4 *>(x + (int64_t)perm[t0 + r] * ld_x + c);
        }
      }
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) {
        const int e = base + k * kAttnThreads;
        if (e < total) {
          const int r = e / d4, c = (e - r * d4) << 2;
          float *o = xs + r * S + c;
          o[0] = v[k].x; o[1] = v[k].y; o[2] = v[k].z; o[3] = v[k].w;
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < rows * dim; e += kAttnThreads) {
      const int r = e / dim, c = e - r * dim;
      xs[r * S + c] = x[(int64_t)perm[t0 + r] * ld_x + c];
    }
  }
}

// s[h] += x_r[d] m[d][h] over the column slice [d0, d1) (and a[h] with m2 when TWO)
template <int HP, bool TWO>
__device__ __forceinline__ void attn_score_walk(const float *__restrict__ xr, const float *__restrict__ m,
                                                const float *__restrict__ m2, int d0, int d1, float (&s)[HP],
                                                float (&a)[HP]) {
  for (int d = d0; d < d1; ++d) {
    const float xv = xr[d];
#pragma unroll
    for (int q = 0; q < HP / 4; ++q) {
      const float4 w = *reinterpret_cast<const float4 *>(m + d * HP + 4 * q);
      s[4 * q + 0] = fmaf(xv, w.x, s[4 * q + 0]);
      s[4 * q + 1] = fmaf(xv, w.y, s[4 * q + 1]);
      s[4 * q + 2] = fmaf(xv, w.z, s[4 * q + 2]);
      s[4 * q + 3] = fmaf(xv, w.w, s[4 * q + 3]);
      if constexpr (TWO) {
        const float4 v = *reinterpret_cast<const float4 *>(m2 + d * HP + 4 * q);
        a[4 * q + 0] = fmaf(xv, v.x, a[4 * q + 0]);
        a[4 * q + 1] = fmaf(xv, v.y, a[4 * q + 1]);
        a[4 * q + 2] = fmaf(xv, v.z, a[4 * q + 2]);
        a[4 * q + 3] = fmaf(xv, v.w, a[4 * q + 3]);
      }
    }
  }
}

// launch `kern` with `lds_bytes` of dynamic LDS, raising its limit first when that is more than the default 64 KiB
template <typename Kern, typename... Args>
int tile_launch(const char *what, Kern kern, size_t lds_bytes, unsigned grid, hipStream_t st, Args... args) {
  PTGNN_REQUIRE(lds_bytes <= 64 * 1024 || raise_dynamic_lds(kern, lds_bytes), PTGNN_AMD_EHIP,
                "%s: %zu bytes of LDS refused", what, lds_bytes);
  kern<<<grid, kAttnThreads, lds_bytes, st>>>(args...);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}
#endif

}  // namespace ptgnn_amd
