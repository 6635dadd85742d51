// The score-free loss of the copying decoder with 16-bit matrix-core inputs (projection_loss.hip is the exact-fp32 pair and
// states the algebra).  What autocast gives an `enable_amp` user of the reference for the vocabulary einsum of
// grucopydecoder.py:111-118: the rows of p [R, E] and T [V, E] rounded to nearest even to bf16 / fp16, their products on
// v_mfma_f32_32x32x16_{bf16,f16} (half16.h's Half16<DT>), and everything else fp32:
//
//     s[r, v]  = rnd(p[r]) . rnd(T[v]) + bias[v]        the fp32 accumulator IS the score: it is never rounded, and the
//                                                       bias, the running (max, sum) and the target pick are fp32
//     G[r, v]  as in projection_loss.hip, fp32, from that accumulator
//     d_bias[v] = sum_r G[r, v], d_extra[r]             fp32 on the unrounded G
//     d_p = rnd(G) rnd(T)      d_T = rnd(G)^T rnd(p)    G rounded ONCE, in registers (ba16_round8)
//
// p, T and every result stay fp32 in memory, any leading dimension and alignment (rows that are not 16-byte aligned take
// the scalar path of ba16_load4).  Ownership, sizes, workspaces and fold orders are those of projection_loss.h, so the
// second launch of the forward is k_vocab_loss_merge and the last of the backward k_projection_loss_fold, unchanged:
//   a.  k_projection_loss16_partial  (64-row block, 256-column chunk) -> (max, sum) partials and the target scores
//   b1. k_projection_loss16_dtable   64 vocabulary columns, walks all rows in row order -> d_T, d_bias complete
//   b2. k_projection_loss16_dproj    (64-row block, 1024-column chunk) -> part[chunk, :, :], d_extra from chunk 0
// A workgroup is 4 waves on 64 x 64 scores at a time, wave w the 32 x 32 tile (w & 1, w >> 1), as in the fp32 file.
//
// LDS images (block_attention16.h says why there are two strides).  E is zero-padded to a multiple of 16 in LDS only.
// A tile that is an operand of the score product is a ROW image at stride ldk = E padded to 16, + 8 elements: both
// operands of a k-step are one ds_read_b128 per lane, 16 MFMAs per score tile at E = 256.  The tile whose row index the
// gradient product sums -- T in dproj, p in dtable -- is parked a second time at stride ldt = 32 (TT | 1) and read
// transposed (ds_read_b64_tr_b16) as the B operand, while the A operand is G straight from the accumulator registers.
//
// Load overlap.  The streamed tile (T and its bias in a and b2; p and the rows' statistics in b1) is fetched into
// registers for step s + 1 BEFORE the products of step s and parked, rounded, AFTER them, with a barrier on either side
// of the park: ONE LDS buffer, and a workgroup small enough for two of them to share a CU wherever the registers allow
// (a at every E; b1 and b2 up to E = 128 by LDS).  That beat the two-buffer image (the other buffer behind one barrier
// per step, one workgroup per CU) that was built and measured beside it at every shape where the two differ
// (profiles/projection_loss16_notes.md), so it is the only walk here.
//
// The two waves of a row (a, b2) / column (b1) tile meet through LDS in a fixed order; no atomics, no inline assembly;
// every result is a fixed function of the shapes and does not depend on strides or alignment.
#include "block_attention16.h"
#include "projection_loss.h"
#include "vocab_loss.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

// A 64-row tile of a [*, dim] fp32 matrix on its way into LDS.  fetch issues this thread's 2 TT row loads (rows srow and
// srow + 32 of the tile, columns 32 t + scol .. + 3; rows past `row_end` repeat the last one and are never stored, columns
// past dim are zeros); park rounds them into the row image and, where there is one, the transposable image.
template <int DT, int TT>
struct Pl16Tile {
  float4 reg[2][TT];

  __device__ __forceinline__ void fetch(const float *__restrict__ src, int64_t ld, int row0, int row_end, int dim,
                                        bool vec) {
    const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      int64_t g = (int64_t)row0 + srow + 32 * half;
      if (g >= row_end) g = row_end - 1;
      const float *row = src + g * ld;
#pragma unroll
      for (int t = 0; t < TT; ++t) reg[half][t] = ba16_load4(row, 32 * t + scol, dim, vec);
    }
  }
  template <bool TR>
  __device__ __forceinline__ void park(uint16_t *rows, int ldk, int ep, uint16_t *tr, int ldt) const {
    const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (32 * t + scol < ep) store4<DT>(rows + (srow + 32 * half) * ldk + 32 * t + scol, reg[half][t]);
        if (TR) store4<DT>(tr + (srow + 32 * half) * ldt + 32 * t + scol, reg[half][t]);
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------------------------
// a. forward
// ------------------------------------------------------------------------------------------------------------------
template <int DT, int TT>
__global__ __launch_bounds__(kPlThreads) void k_projection_loss16_partial(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    int chunks, const float *__restrict__ bias, const int64_t *__restrict__ targets, float2 *__restrict__ partial,
    float *__restrict__ target_score, int vec_p, int vec_t) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  const int ep = ((dim + 15) >> 4) * 16, ldk = ep + 8;
  float *bias_s = reinterpret_cast<float *>(lds16);                         // a step's 64 biases
  MaxSum *other = reinterpret_cast<MaxSum *>(bias_s + kPlStep);             // [64]: the states of the second column waves
  uint16_t *Ps = lds16 + 2 * kPlStep + 4 * kPlRows, *Tr = Ps + kPlRows * ldk;
  const int rb = blockIdx.x / chunks, ck = blockIdx.x % chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int rh = wave & 1, cp = wave >> 1;                                  // the wave's 32 rows / its 32 columns of a step
  const int row0 = rb * kPlRows;
  const int cbeg = ck * kPlFwdCols, cend = min(cbeg + kPlFwdCols, vocab);

  Pl16Tile<DT, TT> tile;
  float breg = 0.0f;
  auto fetch = [&](int col0) {
    tile.fetch(T, ld_t, col0, vocab, dim, vec_t);
    if (threadIdx.x < kPlStep) {
      const int col = col0 + threadIdx.x;
      breg = bias && col < vocab ? bias[col] : 0.0f;
    }
  };
  auto park = [&]() {
    tile.template park<false>(Tr, ldk, ep, nullptr, 0);
    if (threadIdx.x < kPlStep) bias_s[threadIdx.x] = breg;
  };

  tile.fetch(p, ld_p, row0, rows, dim, vec_p);
  tile.template park<false>(Ps, ldk, ep, nullptr, 0);
  fetch(cbeg);
  park();
  __syncthreads();

  const uint16_t *Pw = Ps + (32 * rh + c) * ldk + 8 * h;
  const int ksteps = ep >> 4;
  const int r = row0 + 32 * rh + c;                                         // the lane's row (nothing of it is kept past the end)
  const int64_t tgt = targets && r < rows ? targets[r] : -1;
  MaxSum a{-INFINITY, 0.0f};
  for (int col0 = cbeg; col0 < cend; col0 += kPlStep) {
    const bool more = col0 + kPlStep < cend;
    if (more) fetch(col0 + kPlStep);
    const int t0 = col0 + 32 * cp;
    // S^T[v, r]: lane = row, registers = columns
    f32x16 x = ba16_nt<DT>(Tr + (32 * cp + c) * ldk + 8 * h, Pw, ksteps);
    const float *bs = bias_s + 32 * cp;
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = t0 + ba_row(j, h) < vocab ? x[j] + bs[ba_row(j, h)] : -INFINITY;
    push_tile(a, x);
    if (tgt >= t0 && tgt < t0 + 32 && tgt < vocab) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (t0 + ba_row(j, h) == tgt) target_score[r] = x[j];              // one (lane, register) of the grid meets it
    }
    __syncthreads();                   // everyone is done reading the tile
    if (more) park();
    __syncthreads();                   // the next tile is complete
  }
  a = combine(a, lane_xor(a, 32));
  if (cp == 1 && h == 0) other[32 * rh + c] = a;
  __syncthreads();
  if (cp == 0 && h == 0 && r < rows) {
    a = combine(a, other[32 * rh + c]);
    partial[(int64_t)r * chunks + ck] = make_float2(a.m, a.s);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// b. backward
// ------------------------------------------------------------------------------------------------------------------
// the second waves' 32 x (32 TT) sums of an output tile pair into `Zs` (row stride 32 TT + 1), for the first waves to add
template <int TT>
__device__ __forceinline__ void pl16_leave(float *Zs, const f32x16 (&z)[TT], int h, int c) {
  constexpr int ldz = 32 * TT + 1;
#pragma unroll
  for (int j = 0; j < 16; ++j)
#pragma unroll
    for (int t = 0; t < TT; ++t) Zs[ba_row(j, h) * ldz + 32 * t + c] = z[t][j];
}

// d_T[v0 .. v0 + 63, :] and d_bias[v0 .. v0 + 63], v0 = 64 blockIdx.x
template <int DT, int TT>
__global__ __launch_bounds__(kPlThreads) void k_projection_loss16_dtable(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    const float *__restrict__ bias, const int64_t *__restrict__ targets, const float2 *__restrict__ stats,
    const float *__restrict__ g_norm, const float *__restrict__ g_picked, float *__restrict__ d_T, int64_t ld_dt,
    float *__restrict__ d_bias, int vec_p, int vec_t) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  const int ep = ((dim + 15) >> 4) * 16, ldk = ep + 8;
  constexpr int ldt = ba16_ldv(TT), ldz = 32 * TT + 1;
  // the 64 rows' [M | log_sum | c | g_picked | target], then the second row waves' bias sums
  float *row_s = reinterpret_cast<float *>(lds16), *bsum_s = row_s + 5 * kPlRows;
  uint16_t *Ts = lds16 + 12 * kPlRows, *Pr = Ts + kPlStep * ldk, *Pt = Pr + kPlRows * ldk;   // p by rows, transposable
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int ct = wave & 1, rp = wave >> 1;                                  // the wave's 32 columns / its 32 rows of a step
  const int v0 = blockIdx.x * kPlStep;

  Pl16Tile<DT, TT> tile;
  float4 sreg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);        // M, log_sum, c, g_picked of the row this thread fetches
  int treg = -1;
  auto fetch = [&](int row0) {
    tile.fetch(p, ld_p, row0, rows, dim, vec_p);
    if (threadIdx.x < kPlRows) {
      const int r = row0 + threadIdx.x;
      const bool ok = r < rows;
      const float gp = ok && g_picked ? g_picked[r] : 0.0f;
      const float2 st = ok ? stats[r] : make_float2(INFINITY, 0.0f);
      const int64_t tg = ok && targets ? targets[r] : -1;
      sreg = make_float4(st.x, st.y, ok ? (g_norm ? g_norm[r] : 0.0f) - gp : 0.0f, gp);
      treg = tg >= 0 && tg < vocab ? (int)tg : -1;
    }
  };
  auto park = [&]() {
    tile.template park<true>(Pr, ldk, ep, Pt, ldt);
    if (threadIdx.x < kPlRows) {
      float *s = row_s + threadIdx.x;
      s[0] = sreg.x;
      s[kPlRows] = sreg.y;
      s[2 * kPlRows] = sreg.z;
      s[3 * kPlRows] = sreg.w;
      reinterpret_cast<int *>(s)[4 * kPlRows] = treg;
    }
  };

  tile.fetch(T, ld_t, v0, vocab, dim, vec_t);
  tile.template park<false>(Ts, ldk, ep, nullptr, 0);
  fetch(0);
  park();
  __syncthreads();

  const uint16_t *Tw = Ts + (32 * ct + c) * ldk + 8 * h;
  const int ksteps = ep >> 4, tr_off = ba16_tr_off(lane, ldt);
  const int col = v0 + 32 * ct + c;                                         // the lane's column
  const bool col_ok = col < vocab;
  const float b = bias && col_ok ? bias[col] : 0.0f;
  f32x16 z[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) zero(z[t]);
  float bsum = 0.0f;
  for (int row0 = 0; row0 < rows; row0 += kPlRows) {                        // row order
    const bool more = row0 + kPlRows < rows;
    if (more) fetch(row0 + kPlRows);
    // S[r, v]: lane = column, registers = rows
    f32x16 x = ba16_nt<DT>(Pr + (32 * rp + c) * ldk + 8 * h, Tw, ksteps);
    const float *rM = row_s + 32 * rp, *rL = rM + kPlRows, *rC = rL + kPlRows, *rG = rC + kPlRows;
    const int *rT = reinterpret_cast<const int *>(rG + kPlRows);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = ba_row(j, h);
      const float g = rC[k] * pl_prob(x[j] + b, rM[k], rL[k]) + (rT[k] == col ? rG[k] : 0.0f);
      x[j] = col_ok ? g : 0.0f;
      bsum += x[j];                                                         // the unrounded G
    }
    // d_T[v, :] += sum_r rnd(G[r, v]) rnd(p[r, :])
    ba16_tn<DT, TT, ldt>(z, x, Pt + 32 * rp * ldt + tr_off);
    __syncthreads();                   // everyone is done reading the tile
    if (more) park();
    __syncthreads();                   // the next tile is complete
  }
  bsum += lane_xor(bsum, 32);
  float *Zs = reinterpret_cast<float *>(Pr) + 32 * ct * ldz;                // the p images are free: the second row waves' sums
  if (rp == 1) {
    pl16_leave<TT>(Zs, z, h, c);
    if (h == 0) bsum_s[32 * ct + c] = bsum;
  }
  __syncthreads();
  if (rp != 0) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int v = v0 + 32 * ct + ba_row(j, h);
    if (v >= vocab) continue;
    float *dst = d_T + (int64_t)v * ld_dt;
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (32 * t + c < dim) dst[32 * t + c] = z[t][j] + Zs[ba_row(j, h) * ldz + 32 * t + c];
  }
  if (d_bias && h == 0 && col_ok) d_bias[col] = bsum + bsum_s[32 * ct + c];
}

// part[chunk, row block, :] = rnd(G[row block, chunk]) rnd(T[chunk, :]); d_extra of the row block from chunk 0
template <int DT, int TT>
__global__ __launch_bounds__(kPlThreads) void k_projection_loss16_dproj(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    int chunks, const float *__restrict__ bias, const float *__restrict__ extra, const int64_t *__restrict__ targets,
    const float2 *__restrict__ stats, const float *__restrict__ g_norm, const float *__restrict__ g_picked,
    float *__restrict__ part, float *__restrict__ d_extra, int vec_p, int vec_t) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  const int ep = ((dim + 15) >> 4) * 16, ldk = ep + 8;
  constexpr int ldt = ba16_ldv(TT), ldz = 32 * TT + 1;
  float *bias_s = reinterpret_cast<float *>(lds16);                         // a step's 64 biases
  uint16_t *Ps = lds16 + 2 * kPlStep, *Tr = Ps + kPlRows * ldk, *Tt = Tr + kPlStep * ldk;   // T by rows, transposable
  const int rb = blockIdx.x / chunks, ck = blockIdx.x % chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int rh = wave & 1, cp = wave >> 1;
  const int row0 = rb * kPlRows;
  const int cbeg = ck * kPlBwdCols, cend = min(cbeg + kPlBwdCols, vocab);

  Pl16Tile<DT, TT> tile;
  float breg = 0.0f;
  auto fetch = [&](int col0) {
    tile.fetch(T, ld_t, col0, vocab, dim, vec_t);
    if (threadIdx.x < kPlStep) {
      const int col = col0 + threadIdx.x;
      breg = bias && col < vocab ? bias[col] : 0.0f;
    }
  };
  auto park = [&]() {
    tile.template park<true>(Tr, ldk, ep, Tt, ldt);
    if (threadIdx.x < kPlStep) bias_s[threadIdx.x] = breg;
  };

  tile.fetch(p, ld_p, row0, rows, dim, vec_p);
  tile.template park<false>(Ps, ldk, ep, nullptr, 0);
  fetch(cbeg);
  park();
  __syncthreads();

  const uint16_t *Pw = Ps + (32 * rh + c) * ldk + 8 * h;
  const int ksteps = ep >> 4, tr_off = ba16_tr_off(lane, ldt);
  const int r = row0 + 32 * rh + c;                                         // the lane's row
  const bool ok = r < rows;
  const float gp = ok && g_picked ? g_picked[r] : 0.0f;
  const float cr = ok ? (g_norm ? g_norm[r] : 0.0f) - gp : 0.0f;
  const float2 st = ok ? stats[r] : make_float2(INFINITY, 0.0f);
  const int64_t tgt = ok && targets ? targets[r] : -1;
  if (d_extra && ck == 0 && cp == 0 && h == 0 && ok) {
    const float e = extra ? pl_prob(extra[r], st.x, st.y) : 0.0f;
    d_extra[r] = e == 0.0f ? 0.0f : cr * e;                                 // extra = -inf: an exact zero
  }
  f32x16 z[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) zero(z[t]);
  for (int col0 = cbeg; col0 < cend; col0 += kPlStep) {                     // column order
    const bool more = col0 + kPlStep < cend;
    if (more) fetch(col0 + kPlStep);
    const int t0 = col0 + 32 * cp;
    // S^T[v, r]: lane = row, registers = columns
    f32x16 x = ba16_nt<DT>(Tr + (32 * cp + c) * ldk + 8 * h, Pw, ksteps);
    const float *bs = bias_s + 32 * cp;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int col = t0 + ba_row(j, h);
      const float g = cr * pl_prob(x[j] + bs[ba_row(j, h)], st.x, st.y) + (tgt == col ? gp : 0.0f);
      x[j] = col < vocab ? g : 0.0f;
    }
    // d_p[r, :] += sum_v rnd(G[r, v]) rnd(T[v, :])
    ba16_tn<DT, TT, ldt>(z, x, Tt + 32 * cp * ldt + tr_off);
    __syncthreads();                   // everyone is done reading the tile
    if (more) park();
    __syncthreads();                   // the next tile is complete
  }
  float *Zs = reinterpret_cast<float *>(Tr) + 32 * rh * ldz;                // the T images are free: the second column waves' sums
  if (cp == 1) pl16_leave<TT>(Zs, z, h, c);
  __syncthreads();
  if (cp != 0) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = row0 + 32 * rh + ba_row(j, h);
    if (row >= rows) continue;
    float *dst = part + ((int64_t)ck * rows + row) * dim;
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (32 * t + c < dim) dst[32 * t + c] = z[t][j] + Zs[ba_row(j, h) * ldz + 32 * t + c];
  }
}

// LDS of a kernel: `floats` floats, the workgroup's own row image and the streamed tile as a row image and, in the
// backward (tt > 0), a transposable one -- there the streamed part also holds the [64, 32 tt + 1] floats of the meeting
size_t pl16_lds_bytes(int dim, int floats, int tt) {
  const size_t ldk = ba16_ldk(dim), streamed = sizeof(uint16_t) * kPlStep * (ldk + (tt ? ba16_ldv(tt) : 0));
  const size_t meeting = tt ? sizeof(float) * kPlRows * (32 * tt + 1) : 0;
  return sizeof(float) * floats + sizeof(uint16_t) * kPlRows * ldk + (streamed > meeting ? streamed : meeting);
}

constexpr int kPl16FwdFloats = kPlStep + 2 * kPlRows, kPl16TableFloats = 6 * kPlRows, kPl16ProjFloats = kPlStep;

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_scorefree_loss16_supported(int32_t dim, int32_t dtype) {
  return half16::dtype_ok(dtype) && dim >= 1 && dim <= kPlMaxDim ? 1 : 0;
}

extern "C" int ptgnn_amd_scorefree_loss16(const float *projected, int64_t ld_p, const float *table, int64_t ld_t,
                                          int64_t rows, int32_t vocab, int32_t dim, const float *bias, const float *extra,
                                          const int64_t *targets, float *norm, float *picked, float *stats,
                                          void *workspace, size_t workspace_bytes, int32_t dtype, void *stream_) {
  const char *what = "scorefree_loss16";
  PTGNN_REQUIRE(half16::dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: unknown dtype id %d", what, dtype);
  if (const int rc = pl_check(what, projected, ld_p, table, ld_t, rows, vocab, dim)) return rc;
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(norm && stats && (!targets || picked), PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE(half16::aligned4(projected) && half16::aligned4(table), PTGNN_AMD_EINVAL,
                "%s: projected / table is not 4-byte aligned", what);
  const PlFwdWs w = pl_fwd_workspace(rows, vocab);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, w.bytes)) return rc;
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                PTGNN_AMD_EINVAL, "%s: workspace and stats must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream_;
  const int chunks = (int)pl_fwd_chunks(vocab);
  float2 *partial = carved<float2>(workspace, w.partial);
  float *target_score = carved<float>(workspace, w.target_score);
  const int vec_p = half16::rows16(projected, ld_p) && dim % 4 == 0, vec_t = half16::rows16(table, ld_t) && dim % 4 == 0;
  const size_t bytes = pl16_lds_bytes(dim, kPl16FwdFloats, 0);
  const unsigned grid = (unsigned)(pl_row_blocks(rows) * chunks);
  int rc = PTGNN_AMD_OK;
  half16::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    PL_TILES((dim + 31) / 32, {
      auto kern = k_projection_loss16_partial<DT, TT>;
      if (!ba_lds_ok(kern, bytes)) {
        rc = PTGNN_AMD_EHIP;
        return;
      }
      kern<<<grid, kPlThreads, bytes, st>>>(projected, ld_p, table, ld_t, (int)rows, vocab, dim, chunks, bias, targets,
                                            partial, target_score, vec_p, vec_t);
    })
  });
  PTGNN_REQUIRE(rc == PTGNN_AMD_OK, rc, "%s: %zu bytes of LDS refused", what, bytes);
  PTGNN_LAUNCH_CHECK();
  launch_vocab_loss_merge(partial, target_score, rows, vocab, chunks, extra, targets, norm, picked,
                          reinterpret_cast<float2 *>(stats), st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_PROJECTION_LOSS16);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_scorefree_loss16_backward(const float *projected, int64_t ld_p, const float *table, int64_t ld_t,
                                                   int64_t rows, int32_t vocab, int32_t dim, const float *bias,
                                                   const float *extra, const int64_t *targets, const float *stats,
                                                   const float *g_norm, const float *g_picked, float *grad_projected,
                                                   int64_t ld_gp, float *grad_table, int64_t ld_gt, float *grad_bias,
                                                   float *grad_extra, void *workspace, size_t workspace_bytes,
                                                   int32_t dtype, void *stream_) {
  const char *what = "scorefree_loss16_backward";
  PTGNN_REQUIRE(half16::dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: unknown dtype id %d", what, dtype);
  if (const int rc = pl_check(what, projected, ld_p, table, ld_t, rows, vocab, dim)) return rc;
  PTGNN_REQUIRE(ld_gp >= dim && ld_gt >= dim, PTGNN_AMD_EINVAL, "%s: leading dimension (%lld, %lld) < dim %d", what,
                (long long)ld_gp, (long long)ld_gt, dim);
  if (rows == 0) return PTGNN_AMD_OK;                                      // the caller zeroes grad_table / grad_bias
  PTGNN_REQUIRE(stats && grad_projected && grad_table, PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, PTGNN_AMD_EINVAL, "%s: stats must be 8-byte aligned", what);
  PTGNN_REQUIRE(half16::aligned4(projected) && half16::aligned4(table), PTGNN_AMD_EINVAL,
                "%s: projected / table is not 4-byte aligned", what);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, pl_bwd_workspace(rows, vocab, dim))) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const float2 *row_stats = reinterpret_cast<const float2 *>(stats);
  float *part = static_cast<float *>(workspace);
  const int chunks = (int)pl_bwd_chunks(vocab), tt = (dim + 31) / 32;
  const int vec_p = half16::rows16(projected, ld_p) && dim % 4 == 0, vec_t = half16::rows16(table, ld_t) && dim % 4 == 0;
  const size_t table_bytes = pl16_lds_bytes(dim, kPl16TableFloats, tt);
  const size_t proj_bytes = pl16_lds_bytes(dim, kPl16ProjFloats, tt);
  const unsigned table_grid = (unsigned)(((int64_t)vocab + kPlStep - 1) / kPlStep);
  const unsigned proj_grid = (unsigned)(pl_row_blocks(rows) * chunks);
  int rc = PTGNN_AMD_OK;
  half16::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    PL_TILES(tt, {
      auto table_kern = k_projection_loss16_dtable<DT, TT>;
      auto proj_kern = k_projection_loss16_dproj<DT, TT>;
      if (!ba_lds_ok(table_kern, table_bytes) || !ba_lds_ok(proj_kern, proj_bytes)) {
        rc = PTGNN_AMD_EHIP;
        return;
      }
      table_kern<<<table_grid, kPlThreads, table_bytes, st>>>(projected, ld_p, table, ld_t, (int)rows, vocab, dim, bias,
                                                             targets, row_stats, g_norm, g_picked, grad_table, ld_gt,
                                                             grad_bias, vec_p, vec_t);
      proj_kern<<<proj_grid, kPlThreads, proj_bytes, st>>>(projected, ld_p, table, ld_t, (int)rows, vocab, dim, chunks,
                                                          bias, extra, targets, row_stats, g_norm, g_picked, part,
                                                          grad_extra, vec_p, vec_t);
    })
  });
  PTGNN_REQUIRE(rc == PTGNN_AMD_OK, rc, "%s: %zu / %zu bytes of LDS (table / projected kernel) refused", what,
                table_bytes, proj_bytes);
  PTGNN_LAUNCH_CHECK();
  launch_projection_loss_fold(part, rows, dim, chunks, grad_projected, ld_gp, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_PROJECTION_LOSS16_BACKWARD);
  return PTGNN_AMD_OK;
}
