// The loss of the copying decoder (ptgnn/neuralmodels/sequence/grucopydecoder.py:111-135, 178-181) with the second
// vocabulary Linear INSIDE it: the scores [R, V] are never written, read or differentiated as a matrix.  With R = B L rows
// (one per decoding location), p [R, E] the projected states, T [V, E] the (dropped-out) embedding table and
// s[r, v] = p[r] . T[v] + bias[v],
//
//   a. projection_loss            norm[r]   = logaddexp(log sum_v exp s[r, v], extra[r])      extra = the copy normaliser
//                                 picked[r] = s[r, targets[r]] - norm[r]
//                                 stats[r]  = (M, log_sum), the unrounded pair of vocab_loss.hip
//   b. projection_loss_backward   G[r, v]   = c_r exp((s[r, v] - M_r) - log_sum_r) + g_picked[r] [v == targets[r]]
//                                 c_r = g_norm[r] - g_picked[r]
//                                 d_p = G T      d_T = G^T p      d_bias[v] = sum_r G[r, v]
//                                 d_extra[r] = c_r exp((extra[r] - M_r) - log_sum_r)
//
// Exact fp32 (v_mfma_f32_32x32x2_f32 through the NT / TN products of block_attention.h), no float atomics; every result is
// a fixed function of the shapes.  It is block_attention.hip's algebra with rows = decoding locations, columns =
// vocabulary entries and no value product in the forward: the score tile of a wave lives in one accumulator, and in the
// backward G goes from that accumulator straight into the next product.
//
// Sizes.  A workgroup is 4 waves and always works on 64 x 64 scores at a time: kPlRows = 64 rows of p against kPlStep = 64
// rows of T, both images in LDS as [row][E rounded up to 32, + 1] (zero-padded in LDS only), wave w the 32 x 32 tile
// (w & 1, w >> 1).  E <= kPlMaxDim = 256: two images of 64 x 257 floats are 128.5 KiB of the 160 KiB of a CU.
//   a. k_projection_loss_partial, workgroup (row block, column chunk of kPlFwdCols = 256): p block staged once, the chunk
//      walked in steps of 64 columns.  Per step a wave forms S^T[v, r] (lane = row, registers = 16 of its 32 columns), adds
//      the bias, pushes the 16 scores into the lane's running (max, sum) and leaves s[r, targets[r]] when it meets that
//      column.  At the end the two lane halves, then the two column waves of a row are merged (MaxSum's commutative
//      combine) and (max, sum) goes to partial[r, chunk], the layout k_vocab_loss_merge folds -- the second launch is
//      that kernel itself (vocab_loss.h).  R = 448, V = 20 000: 7 x 79 = 553 workgroups for 256 CUs.
//   b1. k_projection_loss_dtable, workgroup = 64 vocabulary columns (T rows staged once), walks ALL rows in steps of 64 in
//      row order with the rows' (M, log_sum, c, g_picked, target) in LDS: S[r, v] (lane = column, registers = rows) -> G
//      -> TN product with the p tile.  The two row waves of a column tile are added through LDS at the end: d_T[tile] and
//      d_bias[tile] (the lane's own running sum of G) complete in the workgroup, no partials.
//   b2. k_projection_loss_dproj, workgroup (row block, column chunk of kPlBwdCols = 1024): as (a) up to S^T, then G with
//      the lane's own row statistics and the TN product with the T tile; the two column waves are added through LDS and
//      the block's [64, E] goes to part[chunk, :, :].  k_projection_loss_fold adds the chunks IN CHUNK ORDER.  d_extra is
//      written by the workgroups of chunk 0.
// Workspace: forward  8 R ceil(V / 256) + 4 R bytes (chunk partials, target scores);
//            backward 4 ceil(V / 1024) R E bytes (the partials of d_p).  Nothing of R V elements exists anywhere.
//
// Traffic: DESIGN.md, "Projection loss".
#include "block_attention.h"
#include "projection_loss.h"
#include "vocab_loss.h"

namespace ptgnn_amd {
namespace {

// one step's 64 rows of T and their bias (0 without one and past the vocabulary) into LDS
__device__ __forceinline__ void pl_stage_table(float *__restrict__ Ts, float *__restrict__ bias_s, int ld,
                                               const float *__restrict__ T, int64_t ld_t, const float *__restrict__ bias,
                                               int col0, int vocab, int dim, int ep) {
  ba_stage(Ts, ld, T, ld_t, col0, vocab, kPlStep, dim, ep);
  if (threadIdx.x < kPlStep) {
    const int col = col0 + threadIdx.x;
    bias_s[threadIdx.x] = bias && col < vocab ? bias[col] : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// a. forward
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlThreads) void k_projection_loss_partial(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    int chunks, const float *__restrict__ bias, const int64_t *__restrict__ targets, float2 *__restrict__ partial,
    float *__restrict__ target_score) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ep = (dim + 31) / 32 * 32, ld = ep + 1;
  float *Ps = lds, *Ts = Ps + kPlRows * ld, *bias_s = Ts + kPlStep * ld;
  MaxSum *other = reinterpret_cast<MaxSum *>(bias_s + kPlStep);           // [64]: the states of the second column waves
  const int rb = blockIdx.x / chunks, ck = blockIdx.x % chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int rh = wave & 1, cp = wave >> 1;                                // the wave's 32 rows / its 32 columns of a step
  const int row0 = rb * kPlRows;
  ba_stage(Ps, ld, p, ld_p, row0, rows, kPlRows, dim, ep);
  const float *Pw = Ps + 32 * rh * ld;
  const int ksteps = (dim + 1) >> 1;
  const int r = row0 + 32 * rh + c;                                       // the lane's row (nothing of it is kept past the end)
  const int64_t tgt = targets && r < rows ? targets[r] : -1;
  MaxSum a{-INFINITY, 0.0f};
  const int cbeg = ck * kPlFwdCols, cend = min(cbeg + kPlFwdCols, vocab);
  for (int col0 = cbeg; col0 < cend; col0 += kPlStep) {
    __syncthreads();
    pl_stage_table(Ts, bias_s, ld, T, ld_t, bias, col0, vocab, dim, ep);
    __syncthreads();
    const int t0 = col0 + 32 * cp;
    f32x16 x = ba_nt(Ts + 32 * cp * ld, ld, Pw, ld, ksteps, lane);        // S^T[v, r]: lane = row, registers = columns
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = t0 + ba_row(j, h) < vocab ? x[j] + bias_s[32 * cp + ba_row(j, h)] : -INFINITY;
    push_tile(a, x);
    if (tgt >= t0 && tgt < t0 + 32 && tgt < vocab) {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (t0 + ba_row(j, h) == tgt) target_score[r] = x[j];            // one (lane, register) of the grid meets it
    }
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
// d_T[v0 .. v0 + 63, :] and d_bias[v0 .. v0 + 63], v0 = 64 blockIdx.x
template <int TT>
__global__ __launch_bounds__(kPlThreads) void k_projection_loss_dtable(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    const float *__restrict__ bias, const int64_t *__restrict__ targets, const float2 *__restrict__ stats,
    const float *__restrict__ g_norm, const float *__restrict__ g_picked, float *__restrict__ d_T, int64_t ld_dt,
    float *__restrict__ d_bias) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ep = 32 * TT, ld = ep + 1;
  float *Ts = lds, *Ps = Ts + kPlStep * ld;
  float *rM = Ps + kPlRows * ld, *rL = rM + kPlRows, *rC = rL + kPlRows, *rG = rC + kPlRows, *bsum_s = rG + kPlRows;
  int *rT = reinterpret_cast<int *>(bsum_s + kPlStep);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int ct = wave & 1, rp = wave >> 1;                                // the wave's 32 columns / its 32 rows of a step
  const int v0 = blockIdx.x * kPlStep;
  ba_stage(Ts, ld, T, ld_t, v0, vocab, kPlStep, dim, ep);
  const float *Tw = Ts + 32 * ct * ld, *Pw = Ps + 32 * rp * ld;
  const int ksteps = (dim + 1) >> 1;
  const int col = v0 + 32 * ct + c;                                       // the lane's column
  const bool col_ok = col < vocab;
  const float b = bias && col_ok ? bias[col] : 0.0f;
  f32x16 z[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) z[t][j] = 0.0f;
  float bsum = 0.0f;
  for (int row0 = 0; row0 < rows; row0 += kPlRows) {                      // row order
    __syncthreads();
    ba_stage(Ps, ld, p, ld_p, row0, rows, kPlRows, dim, ep);
    if (threadIdx.x < kPlRows) {
      const int k = threadIdx.x, r = row0 + k;
      const bool ok = r < rows;
      const float gp = ok && g_picked ? g_picked[r] : 0.0f;
      const float2 st = ok ? stats[r] : make_float2(INFINITY, 0.0f);
      const int64_t tg = ok && targets ? targets[r] : -1;
      rM[k] = st.x;
      rL[k] = st.y;
      rC[k] = ok ? (g_norm ? g_norm[r] : 0.0f) - gp : 0.0f;
      rG[k] = gp;
      rT[k] = tg >= 0 && tg < vocab ? (int)tg : -1;
    }
    __syncthreads();
    f32x16 x = ba_nt(Pw, ld, Tw, ld, ksteps, lane);                       // S[r, v]: lane = column, registers = rows
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int k = 32 * rp + ba_row(j, h);
      const float g = rC[k] * pl_prob(x[j] + b, rM[k], rL[k]) + (rT[k] == col ? rG[k] : 0.0f);
      x[j] = col_ok ? g : 0.0f;
      bsum += x[j];
    }
    ba_tn<TT>(z, x, Pw, ld, lane);                                        // d_T[v, :] += sum_r G[r, v] p[r, :]
  }
  __syncthreads();
  bsum += lane_xor(bsum, 32);
  float *Zs = Ps + 32 * ct * ld;                                          // the p image is free: the second row waves' sums
  if (rp == 1) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
#pragma unroll
      for (int t = 0; t < TT; ++t) Zs[ba_row(j, h) * ld + 32 * t + c] = z[t][j];
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
      if (32 * t + c < dim) dst[32 * t + c] = z[t][j] + Zs[ba_row(j, h) * ld + 32 * t + c];
  }
  if (d_bias && h == 0 && col_ok) d_bias[col] = bsum + bsum_s[32 * ct + c];
}

// part[chunk, row block, :] = G[row block, chunk] T[chunk, :]; d_extra of the row block from chunk 0
template <int TT>
__global__ __launch_bounds__(kPlThreads) void k_projection_loss_dproj(
    const float *__restrict__ p, int64_t ld_p, const float *__restrict__ T, int64_t ld_t, int rows, int vocab, int dim,
    int chunks, const float *__restrict__ bias, const float *__restrict__ extra, const int64_t *__restrict__ targets,
    const float2 *__restrict__ stats, const float *__restrict__ g_norm, const float *__restrict__ g_picked,
    float *__restrict__ part, float *__restrict__ d_extra) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int ep = 32 * TT, ld = ep + 1;
  float *Ps = lds, *Ts = Ps + kPlRows * ld, *bias_s = Ts + kPlStep * ld;
  const int rb = blockIdx.x / chunks, ck = blockIdx.x % chunks;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int rh = wave & 1, cp = wave >> 1;
  const int row0 = rb * kPlRows;
  ba_stage(Ps, ld, p, ld_p, row0, rows, kPlRows, dim, ep);
  const float *Pw = Ps + 32 * rh * ld, *Tw = Ts + 32 * cp * ld;
  const int ksteps = (dim + 1) >> 1;
  const int r = row0 + 32 * rh + c;                                       // the lane's row
  const bool ok = r < rows;
  const float gp = ok && g_picked ? g_picked[r] : 0.0f;
  const float cr = ok ? (g_norm ? g_norm[r] : 0.0f) - gp : 0.0f;
  const float2 st = ok ? stats[r] : make_float2(INFINITY, 0.0f);
  const int64_t tgt = ok && targets ? targets[r] : -1;
  if (d_extra && ck == 0 && cp == 0 && h == 0 && ok) {
    const float e = extra ? pl_prob(extra[r], st.x, st.y) : 0.0f;
    d_extra[r] = e == 0.0f ? 0.0f : cr * e;                               // extra = -inf: an exact zero
  }
  f32x16 z[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) z[t][j] = 0.0f;
  const int cbeg = ck * kPlBwdCols, cend = min(cbeg + kPlBwdCols, vocab);
  for (int col0 = cbeg; col0 < cend; col0 += kPlStep) {                   // column order
    __syncthreads();
    pl_stage_table(Ts, bias_s, ld, T, ld_t, bias, col0, vocab, dim, ep);
    __syncthreads();
    const int t0 = col0 + 32 * cp;
    f32x16 x = ba_nt(Tw, ld, Pw, ld, ksteps, lane);                       // S^T[v, r]: lane = row, registers = columns
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int col = t0 + ba_row(j, h);
      const float g = cr * pl_prob(x[j] + bias_s[32 * cp + ba_row(j, h)], st.x, st.y) + (tgt == col ? gp : 0.0f);
      x[j] = col < vocab ? g : 0.0f;
    }
    ba_tn<TT>(z, x, Tw, ld, lane);                                        // d_p[r, :] += sum_v G[r, v] T[v, :]
  }
  __syncthreads();
  float *Zs = Ts + 32 * rh * ld;                                          // the T image is free: the second column waves' sums
  if (cp == 1) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
#pragma unroll
      for (int t = 0; t < TT; ++t) Zs[ba_row(j, h) * ld + 32 * t + c] = z[t][j];
  }
  __syncthreads();
  if (cp != 0) return;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = row0 + 32 * rh + ba_row(j, h);
    if (row >= rows) continue;
    float *dst = part + ((int64_t)ck * rows + row) * dim;
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (32 * t + c < dim) dst[32 * t + c] = z[t][j] + Zs[ba_row(j, h) * ld + 32 * t + c];
  }
}

// d_p[r, e] = the column chunks' partials added in chunk order
__global__ __launch_bounds__(kPlThreads) void k_projection_loss_fold(const float *__restrict__ part, int64_t rows, int dim,
                                                                    int chunks, float *__restrict__ d_p, int64_t ld_dp) {
  const int64_t i = (int64_t)blockIdx.x * kPlThreads + threadIdx.x;
  if (i >= rows * dim) return;
  d_p[i / dim * ld_dp + i % dim] = chunk_fold(part + i, rows * dim, 0, chunks);
}

// two 64-row images and `extra` floats
size_t pl_lds_bytes(int32_t dim, int extra) {
  const int ld = (dim + 31) / 32 * 32 + 1;
  return sizeof(float) * ((size_t)(kPlRows + kPlStep) * ld + extra);
}

}  // namespace

void launch_projection_loss_fold(const float *part, int64_t rows, int dim, int chunks, float *d_p, int64_t ld_dp,
                                 hipStream_t st) {
  k_projection_loss_fold<<<(unsigned)((rows * dim + kPlThreads - 1) / kPlThreads), kPlThreads, 0, st>>>(part, rows, dim,
                                                                                                       chunks, d_p, ld_dp);
}

}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_projection_loss_supported(int32_t dim) { return dim >= 1 && dim <= kPlMaxDim ? 1 : 0; }

extern "C" size_t ptgnn_amd_projection_loss_workspace_bytes(int64_t rows, int32_t vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  return pl_fwd_workspace(rows, vocab).bytes;
}

extern "C" int ptgnn_amd_projection_loss_f32(const float *projected, int64_t ld_p, const float *table, int64_t ld_t,
                                             int64_t rows, int32_t vocab, int32_t dim, const float *bias,
                                             const float *extra, const int64_t *targets, float *norm, float *picked,
                                             float *stats, void *workspace, size_t workspace_bytes, void *stream_) {
  const char *what = "projection_loss";
  if (const int rc = pl_check(what, projected, ld_p, table, ld_t, rows, vocab, dim)) return rc;
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(norm && stats && (!targets || picked), PTGNN_AMD_EINVAL, "%s: null pointer", what);
  const PlFwdWs w = pl_fwd_workspace(rows, vocab);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, w.bytes)) return rc;
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                PTGNN_AMD_EINVAL, "%s: workspace and stats must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream_;
  const int chunks = (int)pl_fwd_chunks(vocab);
  float2 *partial = carved<float2>(workspace, w.partial);
  float *target_score = carved<float>(workspace, w.target_score);
  const size_t bytes = pl_lds_bytes(dim, kPlStep + 2 * kPlRows);           // bias of a step, the second waves' states
  PTGNN_REQUIRE(ba_lds_ok(k_projection_loss_partial, bytes), PTGNN_AMD_EHIP, "%s: %zu bytes of LDS refused", what, bytes);
  k_projection_loss_partial<<<(unsigned)(pl_row_blocks(rows) * chunks), kPlThreads, bytes, st>>>(
      projected, ld_p, table, ld_t, (int)rows, vocab, dim, chunks, bias, targets, partial, target_score);
  PTGNN_LAUNCH_CHECK();
  launch_vocab_loss_merge(partial, target_score, rows, vocab, chunks, extra, targets, norm, picked,
                          reinterpret_cast<float2 *>(stats), st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_PROJECTION_LOSS);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_projection_loss_backward_workspace_bytes(int64_t rows, int32_t vocab, int32_t dim) {
  if (rows <= 0 || vocab <= 0 || dim <= 0) return 0;
  return pl_bwd_workspace(rows, vocab, dim);
}

extern "C" int ptgnn_amd_projection_loss_backward_f32(const float *projected, int64_t ld_p, const float *table,
                                                      int64_t ld_t, int64_t rows, int32_t vocab, int32_t dim,
                                                      const float *bias, const float *extra, const int64_t *targets,
                                                      const float *stats, const float *g_norm, const float *g_picked,
                                                      float *grad_projected, int64_t ld_gp, float *grad_table,
                                                      int64_t ld_gt, float *grad_bias, float *grad_extra,
                                                      void *workspace, size_t workspace_bytes, void *stream_) {
  const char *what = "projection_loss_backward";
  if (const int rc = pl_check(what, projected, ld_p, table, ld_t, rows, vocab, dim)) return rc;
  PTGNN_REQUIRE(ld_gp >= dim && ld_gt >= dim, PTGNN_AMD_EINVAL, "%s: leading dimension (%lld, %lld) < dim %d", what,
                (long long)ld_gp, (long long)ld_gt, dim);
  if (rows == 0) return PTGNN_AMD_OK;                                      // the caller zeroes grad_table / grad_bias
  PTGNN_REQUIRE(stats && grad_projected && grad_table, PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, PTGNN_AMD_EINVAL, "%s: stats must be 8-byte aligned", what);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, pl_bwd_workspace(rows, vocab, dim))) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const float2 *row_stats = reinterpret_cast<const float2 *>(stats);
  float *part = static_cast<float *>(workspace);
  const int chunks = (int)pl_bwd_chunks(vocab);
  const size_t table_bytes = pl_lds_bytes(dim, 6 * kPlRows);               // M, log_sum, c, g_picked, target, bias sums
  const size_t proj_bytes = pl_lds_bytes(dim, kPlStep);                    // bias of a step
  const unsigned table_grid = (unsigned)(((int64_t)vocab + kPlStep - 1) / kPlStep);
  const unsigned proj_grid = (unsigned)(pl_row_blocks(rows) * chunks);
  PL_TILES((dim + 31) / 32, {
    auto table_kern = k_projection_loss_dtable<TT>;
    auto proj_kern = k_projection_loss_dproj<TT>;
    PTGNN_REQUIRE(ba_lds_ok(table_kern, table_bytes) && ba_lds_ok(proj_kern, proj_bytes), PTGNN_AMD_EHIP,
                  "%s: %zu bytes of LDS refused", what, table_bytes);
    table_kern<<<table_grid, kPlThreads, table_bytes, st>>>(projected, ld_p, table, ld_t, (int)rows, vocab, dim, bias,
                                                           targets, row_stats, g_norm, g_picked, grad_table, ld_gt,
                                                           grad_bias);
    PTGNN_LAUNCH_CHECK();
    proj_kern<<<proj_grid, kPlThreads, proj_bytes, st>>>(projected, ld_p, table, ld_t, (int)rows, vocab, dim, chunks, bias,
                                                        extra, targets, row_stats, g_norm, g_picked, part, grad_extra);
    PTGNN_LAUNCH_CHECK();
  })
  launch_projection_loss_fold(part, rows, dim, chunks, grad_projected, ld_gp, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_PROJECTION_LOSS_BACKWARD);
  return PTGNN_AMD_OK;
}
