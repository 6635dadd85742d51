// The attention pool of attention_pool.hip and the copy scores of segment_scores.hip for 9 .. 64 heads / vectors per
// sample, on the matrix cores.  Past 8 heads the pass is 2 * heads FLOP per element >= 32 FLOP / B: above the vector ridge
// (19.6 FLOP / B), so the half-wave-per-head FMA walk of those files is the wrong tool; per sample the pool is a small
// cross-attention (queries = the sample's `heads` vectors, keys = values = its rows), and both of its products are
// exact-fp32 v_mfma_f32_32x32x2_f32 tiles here.  The algebra, the contracts (inputs, outputs, stats, overwrite rules)
// and the chunk rule are those files'; only the supported range differs: 9 <= heads <= 64 (wide_supported).
//
// Layout.  A workgroup of 256 threads (4 waves) owns one 128-row chunk (segment_chunks.h) and walks it in tiles of 32
// rows, gathered through perm into xs[32][S] by attention_tile.h's row staging.  S >= dim rounded up to even with
// S = 2 (mod 4): the A-operand read of the score product (lane l: row l & 31, column 2 s + (l >> 5)) then hits 64
// distinct banks, and so does the B-operand read of the second product, whose K step s takes rows s and s + 16
// (16 S = 32 mod 64).  Columns dim .. S - 1 and the rows past the chunk end are zeroed, so padding contributes exact 0.
// HB = 1 or 2 blocks of 32 heads; TPW = the 32-column tiles of D a wave owns (tile w, w + 4, ...; at most 4).
//
// Forward, per tile:
//   1. S[32 x 32 HB] = X U^T.  The four waves split K = D into quarters; each leaves its partial tile in LDS
//      (part[w][32][PS]) and the partials are added in wave order.  U of the segment is staged ONCE per chunk into LDS as
//      [32 HB][S] when the 160 KB allow it (every forward shape of the supported range); otherwise its fragments are
//      read per K step from global memory (L2: the same 64 KB for every chunk of a segment) -- the pool backward at 33 .. 64
//      heads from D = 128 on, and at D > 256.
//   2. thread (head j = t % 32 HB, row group t / 32 HB) adds the partials of its rows, the row groups meet through LDS in
//      a fixed order: tile max, the running (max, sum) of softmax_state.h's MaxSum, p = exp(s - max); padded heads and
//      rows past the chunk end are -inf / p = 0.  Scores mode stores s (coalesced along L) and stops here.
//   3. acc[heads x D] = acc alpha + p^T X: p parked in LDS as [32][PT] is the A operand, the X tile the B operand; the
//      waves split the D columns and keep their HB x TPW accumulator tiles in registers for the whole chunk.
// A chunk leaves (max, sum, acc) per head; the chunks of a segment meet in attention_pool.hip's / segment_scores.hip's
// own merge launch (launch_attn_merge / launch_scores_merge), in chunk order: no float atomics, the same bits wherever
// the segment sits in the batch.
//
// Backward (pool), per tile, from dP and the forward's P and log-sum-exp: S = X U^T is formed as in the forward (the same
// K quarters added in the same order: the same bits, so the recomputed p is the forward's) and a = X dP^T beside it;
// p = exp(S - lse), ds = p (a - abar); dx = p dP + ds U ([32 x heads] [heads x D],
// the waves split the D columns, written in element order) and du += ds^T X as chunk partials folded in chunk order.
// Backward (scores): t = ds_in + dlse exp(scores - lse) from the stored scores (no score product), dy = t V, dV += t^T Y.
#include <math.h>

#include "attention_tile.h"
#include "block_attention.h"
#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {
namespace {

constexpr int kWideMinHeads = kAttnMaxHeads + 1;   // below: the vector kernels' shapes
constexpr int kWideMaxHeads = 64;
constexpr int kWideMaxDim = 512;                   // 16 column tiles: 4 per wave
constexpr int kWideTile = 32;                      // rows of a tile

enum WideMode { kWidePool = 0, kWideScores = 1 };

struct WideLayout {
  int HB, TPW, S, PS, PT;   // head blocks, column tiles per wave, strides of xs / part / the p tile
  bool resident;            // U (and dP) staged in LDS
  size_t bytes;
};

// LDS (floats).  forward: xs [32][S] | part [4][32][PS] | pt [32][PT] | red_m, red_s [256] | alpha [64] | us [32 HB][S]
//                backward: xs | part | part_a [4][32][PS] | pt | dt [32][PT] | red [256] | us, gs [32 HB][S]
//                (scores mode: neither part_a nor gs)
WideLayout wide_layout(int dim, int heads, int mode, bool backward) {
  WideLayout L;
  L.HB = (heads + 31) / 32;
  const int dp = (dim + 1) & ~1;
  L.S = dp % 4 == 0 ? dp + 2 : dp;
  L.TPW = dim <= 128 ? 1 : (dim <= 256 ? 2 : 4);
  const int HP = 32 * L.HB;
  L.PS = HP + 8;
  L.PT = HP + 2;
  size_t fl = (size_t)kWideTile * L.S + 4 * kWideTile * L.PS + (size_t)kWideTile * L.PT;
  fl += backward ? (mode == kWidePool ? 4 * kWideTile * L.PS : 0) + (size_t)kWideTile * L.PT + 256 : 256 + 256 + 64;
  const size_t operands = (size_t)(backward && mode == kWidePool ? 2 : 1) * HP * L.S;
  L.resident = sizeof(float) * (fl + operands) <= kAttnMaxLds;
  L.bytes = sizeof(float) * (fl + (L.resident ? operands : 0));
  return L;
}

bool wide_supported(int dim, int heads) {
  if (heads < kWideMinHeads || heads > kWideMaxHeads || dim < 1 || dim > kWideMaxDim) return false;
  const WideLayout L = wide_layout(dim, heads, kWidePool, true);
  return L.HB * L.TPW <= 4 && L.bytes <= kAttnMaxLds;     // accumulator tiles of a wave: registers, no scratch
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.0f;
  return c;
}

// the [32 HB][S] image of the segment's [heads][dim] rows (padded heads and columns 0)
__device__ __forceinline__ void wide_stage_heads(float *__restrict__ dst, const float *__restrict__ src, int HP, int S,
                                                 int dim, int heads) {
  for (int e = threadIdx.x; e < HP * S; e += kAttnThreads) {
    const int h = e / S, d = e - h * S;
    dst[e] = h < heads && d < dim ? src[(int64_t)h * dim + d] : 0.0f;
  }
}

// the tile's rows into xs, the rows past `rows` zeroed (the pad columns were zeroed once: the staging never writes them)
__device__ __forceinline__ void wide_stage_tile(float *__restrict__ xs, int S, const float *__restrict__ x, int64_t ld_x,
                                                const int32_t *__restrict__ perm, int t0, int rows, int dim, bool vec4) {
  attn_stage_rows(xs, S, x, ld_x, perm, t0, rows, dim, vec4);
  for (int e = rows * S + threadIdx.x; e < kWideTile * S; e += kAttnThreads) xs[e] = 0.0f;
}

// acc[hb][i, j] += sum over the K steps [s0, s1) of xs[i, k] m[32 hb + j, k], k = 2 s + (lane >> 5).  `m` is the LDS
// image (ld = S) or the segment's rows in global memory (ld = dim); the guard keeps a global read inside the rows.
template <int HB>
__device__ __forceinline__ void wide_scores(f32x16 (&acc)[HB], const float *__restrict__ xs, int S, const float *m,
                                            int ldm, int dim, int heads, int s0, int s1, int lane) {
  const int li = lane & 31, lh = lane >> 5;
  const float *a = xs + li * S + lh;
  for (int s = s0; s < s1; ++s) {
    const int k = 2 * s + lh;
    const float av = a[2 * s];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
      const int h = 32 * hb + li;
      const float bv = h < heads && k < dim ? m[(int64_t)h * ldm + k] : 0.0f;
      acc[hb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[hb], 0, 0, 0);
    }
  }
}

template <int HB>
__device__ __forceinline__ void wide_park(float *__restrict__ part, int PS, const f32x16 (&acc)[HB], int lane) {
  const int li = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[ba_row(r, lh) * PS + 32 * hb + li] = acc[hb][r];
}

// z[hb][c][i, j] += sum_r w[r, 32 hb + i] xs[r, 32 tile(c) + j] over the 32 rows of the tile (K step s: rows s, s + 16)
template <int HB, int TPW>
__device__ __forceinline__ void wide_transposed(f32x16 (&z)[HB][TPW], const float *__restrict__ w, int PT,
                                                const float *__restrict__ xs, int S, int dim, int wave, int lane) {
  const int li = lane & 31, lh = lane >> 5;
#pragma unroll 4
  for (int s = 0; s < 16; ++s) {
    const int r = s + 16 * lh;
    float av[HB];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) av[hb] = w[r * PT + 32 * hb + li];
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
      const int col = 32 * (wave + 4 * c) + li;
      if (32 * (wave + 4 * c) >= dim) break;            // wave-uniform: the wave has no such column tile
      const float bv = col < dim ? xs[r * S + col] : 0.0f;
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) z[hb][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[hb], bv, z[hb][c], 0, 0, 0);
    }
  }
}

// the chunk's [heads][dim] accumulator tiles -> dst[h * dim + col]
template <int HB, int TPW>
__device__ __forceinline__ void wide_store_heads(float *__restrict__ dst, const f32x16 (&z)[HB][TPW], int dim, int heads,
                                                 int wave, int lane) {
  const int li = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
      const int col = 32 * (wave + 4 * c) + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int h = 32 * hb + ba_row(r, lh);
        if (h < heads && col < dim) dst[(int64_t)h * dim + col] = z[hb][c][r];
      }
    }
}

template <int MODE, int HB, int TPW>
__global__ __launch_bounds__(kAttnThreads) void k_wide_forward(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ u, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int heads, int S, bool resident, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, float *__restrict__ partial, float *__restrict__ stat_partial,
    float *__restrict__ scores) {
  extern __shared__ float lds[];
  constexpr int HP = 32 * HB, PS = HP + 8, PT = HP + 2, RG = kAttnThreads / HP, RPT = kWideTile / RG;
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  float *xs = lds;
  float *part = xs + kWideTile * S;
  float *pt = part + 4 * kWideTile * PS;
  float *red_m = pt + kWideTile * PT;
  float *red_s = red_m + 256;
  float *alpha_s = red_s + 256;
  float *us = alpha_s + 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float *useg = u + (int64_t)ch.seg * heads * dim;
  if (resident) wide_stage_heads(us, useg, HP, S, dim, heads);
  const float *um = resident ? us : useg;
  const int ldu = resident ? S : dim;
  for (int e = t; e < kWideTile * (S - dim); e += kAttnThreads) {      // the pad columns, once
    const int r = e / (S - dim), c = dim + e % (S - dim);
    xs[r * S + c] = 0.0f;
  }
  const int ksteps = (dim + 1) >> 1, kq = (ksteps + 3) >> 2;
  const int s0 = wave * kq < ksteps ? wave * kq : ksteps, s1 = s0 + kq < ksteps ? s0 + kq : ksteps;
  const int j = t % HP, rg = t / HP;                  // step 2: the thread's head and row group
  MaxSum run{-INFINITY, 0.0f};
  f32x16 acc[HB][TPW];
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int c = 0; c < TPW; ++c) acc[hb][c] = zero16();

  for (int t0 = ch.lo; t0 < ch.hi; t0 += kWideTile) {
    const int rows = ch.hi - t0 < kWideTile ? ch.hi - t0 : kWideTile;
    __syncthreads();                                   // the previous tile's readers are done
    wide_stage_tile(xs, S, x, ld_x, perm, t0, rows, dim, vec4);
    __syncthreads();
    {
      f32x16 sc[HB];
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) sc[hb] = zero16();
      wide_scores<HB>(sc, xs, S, um, ldu, dim, heads, s0, s1, lane);
      wide_park<HB>(part + wave * kWideTile * PS, PS, sc, lane);
    }
    __syncthreads();
    float sv[RPT];
    float tmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = rg * RPT + k;
      float v = -INFINITY;
      if (r < rows && j < heads) {
        v = part[r * PS + j];
        for (int w = 1; w < 4; ++w) v += part[(w * kWideTile + r) * PS + j];
        if (MODE == kWideScores) scores[(int64_t)perm[t0 + r] * heads + j] = v;
      }
      sv[k] = v;
      tmax = fmaxf(tmax, v);
    }
    red_m[rg * HP + j] = tmax;
    __syncthreads();
    float mnew = run.m;
    for (int g = 0; g < RG; ++g) mnew = fmaxf(mnew, red_m[g * HP + j]);
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const float p = sv[k] == -INFINITY ? 0.0f : expf(sv[k] - mnew);
      if (MODE == kWidePool) pt[(rg * RPT + k) * PT + j] = p;
      sum += p;
    }
    red_s[rg * HP + j] = sum;
    const float alpha = raise_max(run, mnew);          // softmax_state.h: the running (max, sum) rescale
    if (MODE == kWidePool && rg == 0) alpha_s[j] = alpha;
    __syncthreads();
    float tsum = 0.0f;
    for (int g = 0; g < RG; ++g) tsum += red_s[g * HP + j];
    run.s += tsum;
    if (MODE == kWidePool) {
      const int lh = lane >> 5;
#pragma unroll
      for (int hb = 0; hb < HB; ++hb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float al = alpha_s[32 * hb + ba_row(r, lh)];
#pragma unroll
          for (int c = 0; c < TPW; ++c) acc[hb][c][r] *= al;
        }
      wide_transposed<HB, TPW>(acc, pt, PT, xs, S, dim, wave, lane);
    }
  }
  if (MODE == kWidePool) wide_store_heads<HB, TPW>(partial + (int64_t)b * heads * dim, acc, dim, heads, wave, lane);
  if (rg == 0 && j < heads) {
    stat_partial[(int64_t)b * 2 * heads + j] = run.m;
    stat_partial[(int64_t)b * 2 * heads + heads + j] = run.s;
  }
}

// MODE pool: a = `pooled`, c = `stats` (the lse half is read), g = dP, e, f unused.
// MODE scores: a = scores, c = lse, g = grad_scores, e = grad_lse.
template <int MODE, int HB, int TPW>
__global__ __launch_bounds__(kAttnThreads) void k_wide_backward(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ u, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int heads, int S, bool resident, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, const float *__restrict__ a_in, const float *__restrict__ c_in,
    const float *__restrict__ g_in, const float *__restrict__ e_in, float *__restrict__ grad_x, int64_t ld_gx,
    float *__restrict__ du_partial) {
  extern __shared__ float lds[];
  constexpr int HP = 32 * HB, PS = HP + 8, PT = HP + 2, RG = kAttnThreads / HP, RPT = kWideTile / RG;
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  float *xs = lds;
  float *part = xs + kWideTile * S;
  float *part_a = part + 4 * kWideTile * PS;
  float *pt = part_a + (MODE == kWidePool ? 4 * kWideTile * PS : 0);
  float *dt = pt + kWideTile * PT;
  float *red = dt + kWideTile * PT;
  float *us = red + 256;
  float *gs = us + HP * S;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const float *useg = u + (int64_t)ch.seg * heads * dim;
  const float *gseg = MODE == kWidePool ? g_in + (int64_t)ch.seg * heads * dim : nullptr;
  if (resident) {
    wide_stage_heads(us, useg, HP, S, dim, heads);
    if (MODE == kWidePool) wide_stage_heads(gs, gseg, HP, S, dim, heads);
  }
  const float *um = resident ? us : useg;
  const float *gm = resident ? gs : gseg;
  const int ldu = resident ? S : dim;
  for (int e = t; e < kWideTile * (S - dim); e += kAttnThreads) {
    const int r = e / (S - dim), c = dim + e % (S - dim);
    xs[r * S + c] = 0.0f;
  }
  const int j = t % HP, rg = t / HP;
  float lse = 0.0f, second = 0.0f;                    // pool: lse, abar; scores: lse, dlse
  if (MODE == kWidePool) {                            // abar = dP[g,h] . P[g,h]: row groups added in a fixed order
    float v = 0.0f;
    if (j < heads) {
      const float *pg = a_in + ((int64_t)ch.seg * heads + j) * dim;
      const float *gg = gseg + (int64_t)j * dim;
      for (int d = rg; d < dim; d += RG) v = fmaf(gg[d], pg[d], v);
      lse = c_in[(int64_t)ch.seg * 2 * heads + heads + j];
    }
    red[rg * HP + j] = v;
    __syncthreads();
    for (int g = 0; g < RG; ++g) second += red[g * HP + j];
  } else if (j < heads) {
    lse = c_in[(int64_t)ch.seg * heads + j];
    second = e_in[(int64_t)ch.seg * heads + j];
  }
  // S = X U^T in the forward's K quarters and wave order -- the same bits, so p = exp(S - lse) sums to the forward's 1
  // -- and a = X dP^T beside it
  const int ksteps = (dim + 1) >> 1, kq = (ksteps + 3) >> 2;
  const int s0 = wave * kq < ksteps ? wave * kq : ksteps, s1 = s0 + kq < ksteps ? s0 + kq : ksteps;
  f32x16 dacc[HB][TPW];
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int c = 0; c < TPW; ++c) dacc[hb][c] = zero16();

  for (int t0 = ch.lo; t0 < ch.hi; t0 += kWideTile) {
    const int rows = ch.hi - t0 < kWideTile ? ch.hi - t0 : kWideTile;
    __syncthreads();
    wide_stage_tile(xs, S, x, ld_x, perm, t0, rows, dim, vec4);
    __syncthreads();
    if (MODE == kWidePool) {
      f32x16 sc[HB];
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) sc[hb] = zero16();
      wide_scores<HB>(sc, xs, S, um, ldu, dim, heads, s0, s1, lane);
      wide_park<HB>(part + wave * kWideTile * PS, PS, sc, lane);
#pragma unroll
      for (int hb = 0; hb < HB; ++hb) sc[hb] = zero16();
      wide_scores<HB>(sc, xs, S, gm, ldu, dim, heads, s0, s1, lane);
      wide_park<HB>(part_a + wave * kWideTile * PS, PS, sc, lane);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = rg * RPT + k;
      float p = 0.0f, ds = 0.0f;
      if (r < rows && j < heads) {
        if (MODE == kWidePool) {
          float sv = part[r * PS + j], av = part_a[r * PS + j];
          for (int w = 1; w < 4; ++w) {
            sv += part[(w * kWideTile + r) * PS + j];
            av += part_a[(w * kWideTile + r) * PS + j];
          }
          p = expf(sv - lse);
          ds = p * (av - second);
        } else {
          const int64_t at = (int64_t)perm[t0 + r] * heads + j;
          ds = fmaf(second, expf(a_in[at] - lse), g_in[at]);
        }
      }
      if (MODE == kWidePool) pt[r * PT + j] = p;
      dt[r * PT + j] = ds;
    }
    __syncthreads();
    // dx[32 x D] = p dP + ds U: K = the heads (step s: heads 2 s, 2 s + 1), the wave's column tiles
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
      const int c0 = 32 * (wave + 4 * c), col = c0 + li;
      if (c0 >= dim) break;                             // wave-uniform
      f32x16 z = zero16();
      for (int s = 0; s < HP / 2; ++s) {
        const int h = 2 * s + lh;
        const bool in = h < heads && col < dim;
        if (MODE == kWidePool) {
          const float gv = in ? gm[(int64_t)h * ldu + col] : 0.0f;
          z = __builtin_amdgcn_mfma_f32_32x32x2f32(pt[li * PT + h], gv, z, 0, 0, 0);
        }
        const float uv = in ? um[(int64_t)h * ldu + col] : 0.0f;
        z = __builtin_amdgcn_mfma_f32_32x32x2f32(dt[li * PT + h], uv, z, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = ba_row(r, lh);
        if (row < rows && col < dim) grad_x[(int64_t)perm[t0 + row] * ld_gx + col] = z[r];
      }
    }
    wide_transposed<HB, TPW>(dacc, dt, PT, xs, S, dim, wave, lane);    // du += ds^T X
  }
  wide_store_heads<HB, TPW>(du_partial + (int64_t)b * heads * dim, dacc, dim, heads, wave, lane);
}

struct WideWorkspace {
  size_t chunk_start, partial, stat_partial, total;
};

// mode: WideMode; forward: the chunk table, (pool) the chunks' [heads, dim] accumulators, the chunks' (max | sum) per
// head; backward: the chunk table and the chunks' [heads, dim] partial rows of du / dv
WideWorkspace wide_workspace(int64_t segments, int64_t elements, int dim, int heads, int mode, bool backward) {
  const size_t bound = (size_t)chunk_count_bound(segments, elements);
  Carve c;
  WideWorkspace w;
  w.chunk_start = c.take(chunk_table_bytes(segments));
  w.partial = backward || mode == kWidePool ? c.take(bound * heads * dim * sizeof(float)) : 0;
  w.stat_partial = backward ? 0 : c.take(bound * 2 * heads * sizeof(float));
  w.total = c.off;
  return w;
}

int wide_check(const char *what, int64_t num_segments, int64_t num_elements, int32_t dim, int32_t num_heads) {
  PTGNN_REQUIRE(num_heads > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  if (const int rc = chunked_segments_check(what, num_segments, num_elements, dim, num_heads)) return rc;
  PTGNN_REQUIRE(wide_supported(dim, num_heads), PTGNN_AMD_EUNSUPPORTED,
                "%s: dim %d / %d heads outside the kernel range (%d <= heads <= %d, dim <= %d; dim <= 256 past 32 heads)",
                what, dim, num_heads, kWideMinHeads, kWideMaxHeads, kWideMaxDim);
  PTGNN_REQUIRE(num_elements <= (((int64_t)1 << 31) - 1) / num_heads, PTGNN_AMD_EUNSUPPORTED,
                "%s: too many segments / elements", what);
  return PTGNN_AMD_OK;
}

// instantiate KERNEL<MODE, HB, TPW> for the layout and launch it
#define WIDE_DISPATCH(RC, WHAT, KERNEL, MODE, L, GRID, ST, ...)                                                      \
  do {                                                                                                                \
    if ((L).HB == 1)                                                                                                  \
      RC = (L).TPW == 1   ? tile_launch(WHAT, KERNEL<MODE, 1, 1>, (L).bytes, GRID, ST, __VA_ARGS__)                   \
           : (L).TPW == 2 ? tile_launch(WHAT, KERNEL<MODE, 1, 2>, (L).bytes, GRID, ST, __VA_ARGS__)                   \
                          : tile_launch(WHAT, KERNEL<MODE, 1, 4>, (L).bytes, GRID, ST, __VA_ARGS__);                  \
    else                                                                                                              \
      RC = (L).TPW == 1 ? tile_launch(WHAT, KERNEL<MODE, 2, 1>, (L).bytes, GRID, ST, __VA_ARGS__)                     \
                        : tile_launch(WHAT, KERNEL<MODE, 2, 2>, (L).bytes, GRID, ST, __VA_ARGS__);                    \
  } while (0)

// the forward of both modes: `out` / `stats` (pool) or `scores` / `lse` (scores)
int wide_forward(const char *what, int mode, const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                 const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim, int32_t heads,
                 float *out, float *stats, void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (const int rc = wide_check(what, num_segments, num_elements, dim, heads)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(u && rowptr && stats && (mode == kWideScores || out) &&
                    (num_elements == 0 || (x && perm && out)), PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE(num_elements == 0 || ld_x >= dim, PTGNN_AMD_EINVAL, "%s: bad leading dimension", what);
  const WideWorkspace ws = wide_workspace(num_segments, num_elements, dim, heads, mode, false);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *partial = carved<float>(workspace, ws.partial);
  float *stat_partial = carved<float>(workspace, ws.stat_partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const WideLayout L = wide_layout(dim, heads, mode, false);     // scores: no column walk, one instantiation per HB
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_x % 4 == 0 && aligned16(x);
  if (bound > 0) {
    int rc = PTGNN_AMD_OK;
    if (mode == kWidePool)
      WIDE_DISPATCH(rc, what, k_wide_forward, kWidePool, L, (unsigned)bound, st, x, ld_x, u, rowptr, perm, (int)dim,
                    (int)heads, L.S, L.resident, (int)num_segments, (const int32_t *)chunk_start, vec4, partial,
                    stat_partial, (float *)nullptr);
    else if (L.HB == 1)
      rc = tile_launch(what, k_wide_forward<kWideScores, 1, 1>, L.bytes, (unsigned)bound, st, x, ld_x, u, rowptr, perm,
                       (int)dim, (int)heads, L.S, L.resident, (int)num_segments, (const int32_t *)chunk_start, vec4,
                       (float *)nullptr, stat_partial, out);
    else
      rc = tile_launch(what, k_wide_forward<kWideScores, 2, 1>, L.bytes, (unsigned)bound, st, x, ld_x, u, rowptr, perm,
                       (int)dim, (int)heads, L.S, L.resident, (int)num_segments, (const int32_t *)chunk_start, vec4,
                       (float *)nullptr, stat_partial, out);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  if (mode == kWidePool)
    launch_attn_merge(partial, stat_partial, chunk_start, dim, heads, num_segments, out, stats, st);
  else
    launch_scores_merge(stat_partial, chunk_start, heads, num_segments, stats, st);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

// the backward of both modes (the argument names of k_wide_backward)
int wide_backward(const char *what, int mode, const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                  const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim, int32_t heads,
                  const float *a_in, const float *c_in, const float *g_in, const float *e_in, float *grad_x,
                  int64_t ld_gx, float *grad_u, void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (const int rc = wide_check(what, num_segments, num_elements, dim, heads)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  const bool pool = mode == kWidePool;
  PTGNN_REQUIRE(u && rowptr && c_in && grad_u && (pool ? a_in && g_in : e_in != nullptr) &&
                    (num_elements == 0 || (x && perm && grad_x && a_in && g_in)),
                PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE(num_elements == 0 || (ld_x >= dim && ld_gx >= dim), PTGNN_AMD_EINVAL, "%s: bad leading dimension", what);
  const WideWorkspace ws = wide_workspace(num_segments, num_elements, dim, heads, mode, true);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *partial = carved<float>(workspace, ws.partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const WideLayout L = wide_layout(dim, heads, mode, true);
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_x % 4 == 0 && aligned16(x);
  if (bound > 0) {
    int rc = PTGNN_AMD_OK;
    if (pool)
      WIDE_DISPATCH(rc, what, k_wide_backward, kWidePool, L, (unsigned)bound, st, x, ld_x, u, rowptr, perm, (int)dim,
                    (int)heads, L.S, L.resident, (int)num_segments, (const int32_t *)chunk_start, vec4, a_in, c_in, g_in,
                    e_in, grad_x, ld_gx, partial);
    else
      WIDE_DISPATCH(rc, what, k_wide_backward, kWideScores, L, (unsigned)bound, st, x, ld_x, u, rowptr, perm, (int)dim,
                    (int)heads, L.S, L.resident, (int)num_segments, (const int32_t *)chunk_start, vec4, a_in, c_in, g_in,
                    e_in, grad_x, ld_gx, partial);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  launch_fold_segments(partial, chunk_start, heads * dim, num_segments, grad_u, (int64_t)heads * dim, st);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_wide_heads_supported(int32_t dim, int32_t num_heads) {
  return wide_supported(dim, num_heads) ? 1 : 0;
}

extern "C" size_t ptgnn_amd_wide_heads_workspace_bytes(int32_t mode, int32_t backward, int64_t num_segments,
                                                       int64_t num_elements, int32_t dim, int32_t num_heads) {
  if (mode < 0 || mode > 1 || num_segments <= 0 || num_elements < 0 || dim <= 0 || num_heads <= 0) return 0;
  return wide_workspace(num_segments, num_elements, dim, num_heads, mode, backward != 0).total;
}

extern "C" int ptgnn_amd_wide_heads_pool_f32(const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                                             const int32_t *perm, int64_t num_segments, int64_t num_elements,
                                             int32_t dim, int32_t num_heads, float *out, float *stats, void *workspace,
                                             size_t workspace_bytes, void *stream) {
  const int rc = wide_forward("wide_heads_pool", kWidePool, x, ld_x, u, rowptr, perm, num_segments, num_elements, dim,
                              num_heads, out, stats, workspace, workspace_bytes, (hipStream_t)stream);
  if (rc == PTGNN_AMD_OK && num_segments > 0) count_launch(PTGNN_AMD_KERNEL_WIDE_HEADS_POOL);
  return rc;
}

extern "C" int ptgnn_amd_wide_heads_pool_backward_f32(const float *x, int64_t ld_x, const float *u,
                                                      const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                                      int64_t num_elements, int32_t dim, int32_t num_heads,
                                                      const float *pooled, const float *stats, const float *grad_out,
                                                      float *grad_x, int64_t ld_gx, float *grad_u, void *workspace,
                                                      size_t workspace_bytes, void *stream) {
  const int rc = wide_backward("wide_heads_pool_backward", kWidePool, x, ld_x, u, rowptr, perm, num_segments,
                               num_elements, dim, num_heads, pooled, stats, grad_out, nullptr, grad_x, ld_gx, grad_u,
                               workspace, workspace_bytes, (hipStream_t)stream);
  if (rc == PTGNN_AMD_OK && num_segments > 0) count_launch(PTGNN_AMD_KERNEL_WIDE_HEADS_POOL_BACKWARD);
  return rc;
}

extern "C" int ptgnn_amd_wide_heads_scores_f32(const float *y, int64_t ld_y, const float *v, const int32_t *rowptr,
                                               const int32_t *perm, int64_t num_segments, int64_t num_elements,
                                               int32_t dim, int32_t num_vectors, float *scores, float *lse,
                                               void *workspace, size_t workspace_bytes, void *stream) {
  const int rc = wide_forward("wide_heads_scores", kWideScores, y, ld_y, v, rowptr, perm, num_segments, num_elements,
                              dim, num_vectors, scores, lse, workspace, workspace_bytes, (hipStream_t)stream);
  if (rc == PTGNN_AMD_OK && num_segments > 0) count_launch(PTGNN_AMD_KERNEL_WIDE_HEADS_SCORES);
  return rc;
}

extern "C" int ptgnn_amd_wide_heads_scores_backward_f32(const float *y, int64_t ld_y, const float *v,
                                                        const int32_t *rowptr, const int32_t *perm,
                                                        int64_t num_segments, int64_t num_elements, int32_t dim,
                                                        int32_t num_vectors, const float *scores, const float *lse,
                                                        const float *grad_scores, const float *grad_lse, float *grad_y,
                                                        int64_t ld_gy, float *grad_v, void *workspace,
                                                        size_t workspace_bytes, void *stream) {
  const int rc = wide_backward("wide_heads_scores_backward", kWideScores, y, ld_y, v, rowptr, perm, num_segments,
                               num_elements, dim, num_vectors, scores, lse, grad_scores, grad_lse, grad_y, ld_gy, grad_v,
                               workspace, workspace_bytes, (hipStream_t)stream);
  if (rc == PTGNN_AMD_OK && num_segments > 0) count_launch(PTGNN_AMD_KERNEL_WIDE_HEADS_SCORES_BACKWARD);
  return rc;
}
