// The copy attention of GruCopyingDecoder (ptgnn/neuralmodels/sequence/grucopydecoder.py:83-97,122-124), the decoder of
// the Graph2Seq task: every memory row is dotted with the L decoder states of ITS sample, and the scores of a sample are
// log-sum-exp'ed per decoding step.  With g the sample of row i and v[g, l, :] the sample's vectors:
//     scores[i, l] = v[g(i), l, :] . y_i                            [n, Lv]   (element order)
//     lse[g, l]    = log sum_{i in g} exp(scores[i, l])             [G, Lv]   (-inf for a sample without rows: eps = 0)
// The reference gathers output_states[input_memories_origin_idx] into [n, L, H] (3.5 KB per row at L = 7, H = 128, next
// to the 512-byte row) for the einsum and runs scatter_logsumexp over the [n, L] scores as five more passes; here y is
// read once and n * Lv + G * Lv floats are written.  Dropout sits between the copy Linear and the dot product, so while
// it is active the rows are C = dropout(W_c x) and the vectors the GRU states; otherwise W_c moves onto the samples
// (v = W_c^T o, [G, L, Dm]) and the rows are the memories themselves -- the same kernel either way.
//
// Layout.  Segments are cut into the 128-row chunks of segment_chunks.h (chunk_locate, the chunk table, the chunk-order
// fold); a workgroup walks one chunk in the row tiles of attention_tile.h -- the staging of rows and vectors and the score
// walk are the attention pool's.  Per tile half-wave l owns vector l: it adds the parts of up to 64 rows in a fixed
// order, writes their scores and folds them into its running (max, sum), so scores spanning more than 100 do not
// overflow.  A chunk leaves (max, sum) per vector; k_scores_merge combines the chunks of a segment in chunk order.  No
// float atomics: a sample's lse has the same bits alone and inside a batch.
//
// Backward, from ds = dL/dscores, dlse = dL/dlse and the forward's scores and lse (no second score walk):
//     t[i, l]    = ds[i, l] + dlse[g, l] exp(scores[i, l] - lse[g, l])
//     dy_i       = sum_l t[i, l] v[g, l, :]                          every row of the plan is written
//     dv[g, l,:] = sum_{i in g} t[i, l] y_i                          chunk partials folded in chunk order, 0 when empty
// one more pass over y with the same chunks and tiles: thread t owns columns t, t + 256, ...
//
// Supported: 1 <= Lv <= 8, 1 <= K <= 1024 (LDS up to 105 KiB at K = 1024, 8 vectors); other shapes answer
// PTGNN_AMD_EUNSUPPORTED and the host composes the reference's operator sequence from the other HIP entry points.
#include <math.h>

#include "attention_tile.h"
#include "segment_chunks.h"

namespace ptgnn_amd {
namespace {

struct ScoreLayout {
  int R, S, HP, cols;   // tile rows, LDS row stride, vectors padded to a float4, columns per thread of the column walk
  size_t bytes;         // dynamic LDS of one workgroup
};

// R: the largest of 64 / 32 / 16 whose LDS image fits 64 KiB, else 16 (launched with a raised LDS limit)
ScoreLayout score_layout(int dim, int vectors, bool backward) {
  ScoreLayout L;
  L.HP = vectors <= 4 ? 4 : 8;
  L.S = dim | 1;
  L.cols = dim <= 256 ? 1 : (dim <= 512 ? 2 : 4);
  for (L.R = 64;; L.R >>= 1) {
    const size_t rest = backward ? (size_t)L.R * L.HP : (size_t)dim * L.HP + (size_t)kAttnThreads * L.HP;
    L.bytes = sizeof(float) * ((size_t)L.R * L.S + rest);
    if (L.bytes <= 64 * 1024 || L.R == 16) break;
  }
  return L;
}

// LDS (floats): xs [R][S] | vt [dim][HP] | part [256][HP]
template <int HP>
__global__ __launch_bounds__(kAttnThreads) void k_scores_partial(
    const float *__restrict__ y, int64_t ld_y, const float *__restrict__ v, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int vectors, int R, int S, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, float *__restrict__ scores, float *__restrict__ stat_partial) {
  extern __shared__ float lds[];
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  const int parts = kAttnThreads / R;
  float *xs = lds;
  float *vt = xs + R * S;
  float *part = vt + dim * HP;
  const int t = threadIdx.x;
  attn_stage_heads<HP>(vt, v + (int64_t)ch.seg * vectors * dim, dim, vectors);
  // score walk: thread t dots row t % R over the column slice of part t / R
  const int wr = t % R, wp = t / R;
  const int slice = (dim + parts - 1) / parts;
  const int d0 = wp * slice < dim ? wp * slice : dim, d1 = d0 + slice < dim ? d0 + slice : dim;
  // half-wave hh owns vector hh: its running max / sum over the chunk (uniform over the half-wave)
  const int hh = t >> 5, hl = t & 31;
  float m_run = -INFINITY, l_run = 0.0f;

  for (int t0 = ch.lo; t0 < ch.hi; t0 += R) {
    const int rows = ch.hi - t0 < R ? ch.hi - t0 : R;
    __syncthreads();                                   // the previous tile's readers are done
    attn_stage_rows(xs, S, y, ld_y, perm, t0, rows, dim, vec4);
    __syncthreads();
    {
      float s[HP], a[HP];
#pragma unroll
      for (int h = 0; h < HP; ++h) s[h] = a[h] = 0.0f;
      if (wr < rows) attn_score_walk<HP, false>(xs + wr * S, vt, nullptr, d0, d1, s, a);
#pragma unroll
      for (int q = 0; q < HP / 4; ++q)
        *reinterpret_cast<float4 *>(part + (wp * R + wr) * HP + 4 * q) =
            make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
    }
    __syncthreads();
    if (hh < vectors) {
      float sc[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = hl + 32 * k;
        sc[k] = -INFINITY;
        if (r < rows) {
          float sv = 0.0f;
          for (int p = 0; p < parts; ++p) sv += part[(p * R + r) * HP + hh];
          sc[k] = sv;
          scores[(int64_t)perm[t0 + r] * vectors + hh] = sv;
        }
      }
      const float mnew = fmaxf(m_run, group_max<32>(fmaxf(sc[0], sc[1])));
      const float alpha = m_run == -INFINITY ? 0.0f : expf(m_run - mnew);
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < 2; ++k) sum += hl + 32 * k < rows ? expf(sc[k] - mnew) : 0.0f;
      l_run = fmaf(l_run, alpha, group_sum<32>(sum));
      m_run = mnew;
    }
  }
  if (hh < vectors && hl == 0) {
    stat_partial[(int64_t)b * 2 * vectors + hh] = m_run;
    stat_partial[(int64_t)b * 2 * vectors + vectors + hh] = l_run;
  }
}

// lse[g,l] = M + log sum_c l_c e^(m_c - M) over the chunks c of g in chunk order, M = max_c m_c; -inf for an empty segment
__global__ __launch_bounds__(256) void k_scores_merge(const float *__restrict__ stat_partial,
                                                       const int32_t *__restrict__ chunk_start, int vectors,
                                                       int64_t segments, float *__restrict__ lse) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segments * vectors) return;
  const int l = (int)(i % vectors);
  const int64_t g = i / vectors;
  const int c0 = chunk_start[g], c1 = chunk_start[g + 1];
  float M = -INFINITY;
  for (int c = c0; c < c1; ++c) M = fmaxf(M, stat_partial[(int64_t)c * 2 * vectors + l]);
  float L = 0.0f;
  for (int c = c0; c < c1; ++c)
    L = fmaf(stat_partial[(int64_t)c * 2 * vectors + vectors + l], expf(stat_partial[(int64_t)c * 2 * vectors + l] - M), L);
  lse[i] = c0 == c1 ? -INFINITY : M + logf(L);
}

// LDS (floats): xs [R][S] | tt [R][HP]
template <int HP, int COLS>
__global__ __launch_bounds__(kAttnThreads) void k_scores_backward(
    const float *__restrict__ y, int64_t ld_y, const float *__restrict__ v, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int vectors, int R, int S, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, const float *__restrict__ scores, const float *__restrict__ lse,
    const float *__restrict__ grad_scores, const float *__restrict__ grad_lse, float *__restrict__ grad_y, int64_t ld_gy,
    float *__restrict__ dv_partial) {
  extern __shared__ float lds[];
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  float *xs = lds;
  float *tt = xs + R * S;
  const int t = threadIdx.x;
  const float *vseg = v + (int64_t)ch.seg * vectors * dim;
  float vc[HP][COLS], dacc[HP][COLS];                   // the thread's columns of v, its dv accumulators
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int col = t + c * kAttnThreads;
      vc[h][c] = h < vectors && col < dim ? vseg[(int64_t)h * dim + col] : 0.0f;
      dacc[h][c] = 0.0f;
    }

  for (int t0 = ch.lo; t0 < ch.hi; t0 += R) {
    const int rows = ch.hi - t0 < R ? ch.hi - t0 : R;
    __syncthreads();
    attn_stage_rows(xs, S, y, ld_y, perm, t0, rows, dim, vec4);
    for (int e = t; e < R * HP; e += kAttnThreads) {    // t[r, h] of the tile (padded vectors and rows 0)
      const int r = e / HP, h = e % HP;
      float tv = 0.0f;
      if (r < rows && h < vectors) {
        const int64_t at = (int64_t)perm[t0 + r] * vectors + h;
        const int64_t gl = (int64_t)ch.seg * vectors + h;
        tv = fmaf(grad_lse[gl], expf(scores[at] - lse[gl]), grad_scores[at]);
      }
      tt[e] = tv;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      float tr[HP];
#pragma unroll
      for (int q = 0; q < HP / 4; ++q) {
        const float4 w = *reinterpret_cast<const float4 *>(tt + r * HP + 4 * q);
        tr[4 * q] = w.x; tr[4 * q + 1] = w.y; tr[4 * q + 2] = w.z; tr[4 * q + 3] = w.w;
      }
      float *gyr = grad_y + (int64_t)perm[t0 + r] * ld_gy;
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        const int col = t + c * kAttnThreads;
        if (col < dim) {
          const float xv = xs[r * S + col];
          float gy = 0.0f;
#pragma unroll
          for (int h = 0; h < HP; ++h) {
            gy = fmaf(tr[h], vc[h][c], gy);
            dacc[h][c] = fmaf(tr[h], xv, dacc[h][c]);
          }
          gyr[col] = gy;
        }
      }
    }
  }
  float *out = dv_partial + (int64_t)b * vectors * dim;  // [chunks][vectors][dim], the chunks of a segment consecutive
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int col = t + c * kAttnThreads;
      if (h < vectors && col < dim) out[h * dim + col] = dacc[h][c];
    }
}

bool scores_supported(int dim, int vectors) {
  return vectors >= 1 && vectors <= kAttnMaxHeads && dim >= 1 && dim <= kAttnMaxDim &&
         score_layout(dim, vectors, false).bytes <= kAttnMaxLds && score_layout(dim, vectors, true).bytes <= kAttnMaxLds;
}

// forward: the chunk table and the chunks' (max | sum) per vector; backward: the chunk table and the chunks' [vectors, dim]
// partial rows of dv
struct ScoreWorkspace {
  size_t chunk_start, partial, total;
};

ScoreWorkspace score_workspace(int64_t segments, int64_t elements, int dim, int vectors, bool backward) {
  const size_t bound = (size_t)chunk_count_bound(segments, elements);
  Carve c;
  ScoreWorkspace w;
  w.chunk_start = c.take(chunk_table_bytes(segments));
  w.partial = c.take(bound * vectors * (backward ? (size_t)dim : 2) * sizeof(float));
  w.total = c.off;
  return w;
}

// the argument checks the forward and the backward share; 0 when the arguments are fine
int scores_check(const char *what, int64_t num_segments, int64_t num_elements, int32_t dim, int32_t num_vectors) {
  PTGNN_REQUIRE(num_vectors > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  if (const int rc = chunked_segments_check(what, num_segments, num_elements, dim, num_vectors)) return rc;
  PTGNN_REQUIRE(scores_supported(dim, num_vectors), PTGNN_AMD_EUNSUPPORTED,
                "%s: dim %d / %d vectors outside the kernel range (dim <= %d, vectors <= %d)", what, dim, num_vectors,
                kAttnMaxDim, kAttnMaxHeads);
  PTGNN_REQUIRE(num_elements <= (((int64_t)1 << 31) - 1) / num_vectors, PTGNN_AMD_EUNSUPPORTED,
                "%s: too many segments / elements", what);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_segment_scores_supported(int32_t dim, int32_t num_vectors) {
  return scores_supported(dim, num_vectors) ? 1 : 0;
}

extern "C" size_t ptgnn_amd_segment_scores_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                           int32_t num_vectors) {
  if (num_segments <= 0 || num_elements < 0 || dim <= 0 || num_vectors <= 0) return 0;
  return score_workspace(num_segments, num_elements, dim, num_vectors, false).total;
}

extern "C" int ptgnn_amd_segment_scores_f32(const float *y, int64_t ld_y, const float *v, const int32_t *rowptr,
                                            const int32_t *perm, int64_t num_segments, int64_t num_elements,
                                            int32_t dim, int32_t num_vectors, float *scores, float *lse,
                                            void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = scores_check("segment_scores", num_segments, num_elements, dim, num_vectors)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(v && rowptr && lse && (num_elements == 0 || (y && perm && scores)), PTGNN_AMD_EINVAL,
                "segment_scores: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || ld_y >= dim, PTGNN_AMD_EINVAL, "segment_scores: bad leading dimension");
  const ScoreWorkspace ws = score_workspace(num_segments, num_elements, dim, num_vectors, false);
  if (const int rc = workspace_check("segment_scores", workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *stat_partial = carved<float>(workspace, ws.partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const ScoreLayout L = score_layout(dim, num_vectors, false);
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_y % 4 == 0 && aligned16(y);
  if (bound > 0) {
    const int rc =
        L.HP == 4 ? tile_launch("segment_scores", k_scores_partial<4>, L.bytes, (unsigned)bound, st, y, ld_y, v, rowptr,
                                perm, (int)dim, (int)num_vectors, L.R, L.S, (int)num_segments,
                                (const int32_t *)chunk_start, vec4, scores, stat_partial)
                  : tile_launch("segment_scores", k_scores_partial<8>, L.bytes, (unsigned)bound, st, y, ld_y, v, rowptr,
                                perm, (int)dim, (int)num_vectors, L.R, L.S, (int)num_segments,
                                (const int32_t *)chunk_start, vec4, scores, stat_partial);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  const int64_t total = num_segments * num_vectors;
  k_scores_merge<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(stat_partial, chunk_start, num_vectors, num_segments,
                                                                   lse);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_SEGMENT_SCORES);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_segment_scores_backward_workspace_bytes(int64_t num_segments, int64_t num_elements,
                                                                    int32_t dim, int32_t num_vectors) {
  if (num_segments <= 0 || num_elements < 0 || dim <= 0 || num_vectors <= 0) return 0;
  return score_workspace(num_segments, num_elements, dim, num_vectors, true).total;
}

// instantiate k_scores_backward<HP, COLS> for the layout and launch it
#define SCORES_BACKWARD(HP_, COLS_)                                                                                    \
  tile_launch("segment_scores_backward", k_scores_backward<HP_, COLS_>, L.bytes, (unsigned)bound, st, y, ld_y, v, rowptr, \
              perm, (int)dim, (int)num_vectors, L.R, L.S, (int)num_segments, (const int32_t *)chunk_start, vec4, scores, \
              lse, grad_scores, grad_lse, grad_y, ld_gy, partial)

extern "C" int ptgnn_amd_segment_scores_backward_f32(const float *y, int64_t ld_y, const float *v,
                                                     const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                                     int64_t num_elements, int32_t dim, int32_t num_vectors,
                                                     const float *scores, const float *lse, const float *grad_scores,
                                                     const float *grad_lse, float *grad_y, int64_t ld_gy, float *grad_v,
                                                     void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = scores_check("segment_scores_backward", num_segments, num_elements, dim, num_vectors)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(v && rowptr && lse && grad_lse && grad_v &&
                    (num_elements == 0 || (y && perm && scores && grad_scores && grad_y)),
                PTGNN_AMD_EINVAL, "segment_scores_backward: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || (ld_y >= dim && ld_gy >= dim), PTGNN_AMD_EINVAL,
                "segment_scores_backward: bad leading dimension");
  const ScoreWorkspace ws = score_workspace(num_segments, num_elements, dim, num_vectors, true);
  if (const int rc = workspace_check("segment_scores_backward", workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *partial = carved<float>(workspace, ws.partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const ScoreLayout L = score_layout(dim, num_vectors, true);
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_y % 4 == 0 && aligned16(y);
  if (bound > 0) {
    int rc;
    if (L.HP == 4)
      rc = L.cols == 1 ? SCORES_BACKWARD(4, 1) : L.cols == 2 ? SCORES_BACKWARD(4, 2) : SCORES_BACKWARD(4, 4);
    else
      rc = L.cols == 1 ? SCORES_BACKWARD(8, 1) : L.cols == 2 ? SCORES_BACKWARD(8, 2) : SCORES_BACKWARD(8, 4);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  launch_fold_segments(partial, chunk_start, num_vectors * dim, num_segments, grad_v, (int64_t)num_vectors * dim, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_SEGMENT_SCORES_BACKWARD);
  return PTGNN_AMD_OK;
}
