// SelfAttentionVarSizedElementReduce and MultiheadSelfAttentionVarSizedElementReduce
// (ptgnn/neuralmodels/reduceops/varsizedsummary.py:84-178), the node -> graph summariser of the Graph2Seq task
// (graph2seq/graph2seq.py:56-66,116-122: D = hidden = 256, 8 heads, a `max` query).
//
// The key Linear commutes with the pooling.  With g the sample of element i, h a head, dk = hidden / heads and c the
// score scale (1 / sqrt(dk) multi-head, 1 single-head):
//     u[g,h,:] = c * W_k[h*dk:(h+1)*dk, :]^T q[g, h*dk:(h+1)*dk]      [G, heads, D]   (k_head_expand)
//     s[i,h]   = u[g(i),h,:] . x_i
//     p[i,h]   = softmax of s[., h] over the elements of g(i)          (exp(scatter_log_softmax(eps=0)))
//     P[g,h,:] = sum_{i in g} p[i,h] x_i                               [G, heads, D]   (this file: ONE pass over x)
// and the value / output Linears run on the [G, ...] pools.  The reference materialises keys [N, hidden] and the weighted
// rows [N, heads * D] (8 KB per node at Graph2Seq's shape); here x is read once and G * heads * D floats are written.
//
// Layout of the pool.  Segments are cut into the 128-row chunks of segment_chunks.h (counted from each segment's own
// start; chunk_locate, the chunk table and the chunk-order fold are that header's); a workgroup walks one chunk in
// tiles of R rows staged through LDS (row stride D | 1: odd, so lanes reading 32 different rows at one column hit 32
// different banks).  Per tile:
//   1. score walk: thread (row r, part) dots ITS column slice of x_r with every head's u (u in LDS as [D][HP], read as
//      broadcast float4): each x element read from LDS feeds HP FMAs, no cross-lane reduction;
//   2. half-wave h owns head h: adds the parts of up to 64 rows in a fixed order, takes the tile max with 5 shuffles,
//      rescales its running (max, sum) -- the online softmax -- and writes the tile's probabilities;
//   3. column walk: thread t owns columns t, t + 256, ...: acc[h] = acc[h] * alpha[h] + sum_r p[r,h] x[r, col].
// A chunk leaves (max, sum, acc) per head; k_attn_merge combines the chunks of a segment in chunk order.  No float
// atomics: a segment's result is a fixed function of its rows and their order, wherever it sits in the batch.
// Work per element: 2 * heads FMAs (score + accumulate), 16 FLOP per 4-byte element at 8 heads -- below the FP32 vector
// ridge of 157 TF / 8 TB/s = 19.6 FLOP / B, so the pool is meant to stream at HBM speed; what it reaches is measured in
// profiles/attnpool_notes.md.
//
// Backward, from dP = dL/dP and the forward's per-(g,h) log-sum-exp (stats):
//     a[i,h] = dP[g,h] . x_i,   abar[g,h] = dP[g,h] . P[g,h],   ds[i,h] = p[i,h] (a[i,h] - abar[g,h])
//     dx_i   = sum_h p[i,h] dP[g,h] + ds[i,h] u[g,h]          du[g,h] = sum_{i in g} ds[i,h] x_i
// one more pass over x with the same chunks and tiles (the score walk dots u and dP at once), dx written in element
// order, du as chunk partials folded in chunk order.  dq and dW_k follow from du through k_head_contract /
// k_head_weight_grad (the Python autograd node of the projection).
//
// Supported: 1 <= heads <= 8, 1 <= D <= 1024 (LDS up to 148 KiB at D = 1024, 8 heads, backward); other shapes answer
// PTGNN_AMD_EUNSUPPORTED and the host composes the reference's operator sequence from the other HIP entry points.
#include <math.h>

#include "attention_tile.h"
#include "segment_chunks.h"

namespace ptgnn_amd {
namespace {

struct AttnLayout {
  int R, S, HP, cols;   // tile rows, LDS row stride, heads padded to a float4, columns per thread of the column walk
  size_t bytes;         // dynamic LDS of one workgroup
};

// R: the largest of 64 / 32 / 16 whose LDS image fits 64 KiB, else 16 (launched with a raised LDS limit)
AttnLayout attn_layout(int dim, int heads, bool backward) {
  AttnLayout L;
  L.HP = heads <= 4 ? 4 : 8;
  L.S = dim | 1;
  L.cols = dim <= 256 ? 1 : (dim <= 512 ? 2 : 4);
  const size_t sets = backward ? 2 : 1;
  for (L.R = 64;; L.R >>= 1) {
    L.bytes = sizeof(float) * ((size_t)L.R * L.S +
                               sets * ((size_t)dim * L.HP + (size_t)kAttnThreads * L.HP + (size_t)L.R * L.HP) +
                               kAttnMaxHeads);
    if (L.bytes <= 64 * 1024 || L.R == 16) break;
  }
  return L;
}

// LDS (floats): xs [R][S] | ut [dim][HP] | part [256][HP] | pt [R][HP] | alpha [8]
template <int HP, int COLS>
__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_partial(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ u, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int heads, int R, int S, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, float *__restrict__ partial, float *__restrict__ stat_partial) {
  extern __shared__ float lds[];
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  const int parts = kAttnThreads / R;
  float *xs = lds;
  float *ut = xs + R * S;
  float *part = ut + dim * HP;
  float *pt = part + kAttnThreads * HP;
  float *alpha_s = pt + R * HP;
  const int t = threadIdx.x;
  attn_stage_heads<HP>(ut, u + (int64_t)ch.seg * heads * dim, dim, heads);
  for (int e = t; e < R * HP; e += kAttnThreads) pt[e] = 0.0f;     // padded heads stay 0
  if (t < kAttnMaxHeads) alpha_s[t] = 0.0f;
  // score walk: thread t dots row t % R over the column slice of part t / R
  const int wr = t % R, wp = t / R;
  const int slice = (dim + parts - 1) / parts;
  const int d0 = wp * slice < dim ? wp * slice : dim, d1 = d0 + slice < dim ? d0 + slice : dim;
  // half-wave hh owns head hh: its running max / sum over the chunk (uniform over the half-wave)
  const int hh = t >> 5, hl = t & 31;
  float m_run = -INFINITY, l_run = 0.0f;
  float acc[HP][COLS];
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) acc[h][c] = 0.0f;

  for (int t0 = ch.lo; t0 < ch.hi; t0 += R) {
    const int rows = ch.hi - t0 < R ? ch.hi - t0 : R;
    __syncthreads();                                   // the previous tile's readers are done
    attn_stage_rows(xs, S, x, ld_x, perm, t0, rows, dim, vec4);
    __syncthreads();
    {
      float s[HP], a[HP];
#pragma unroll
      for (int h = 0; h < HP; ++h) s[h] = a[h] = 0.0f;
      if (wr < rows) attn_score_walk<HP, false>(xs + wr * S, ut, nullptr, d0, d1, s, a);
#pragma unroll
      for (int q = 0; q < HP / 4; ++q)
        *reinterpret_cast<float4 *>(part + (wp * R + wr) * HP + 4 * q) =
            make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
    }
    __syncthreads();
    if (hh < heads) {
      float sc[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = hl + 32 * k;
        sc[k] = -INFINITY;
        if (r < rows) {
          float v = 0.0f;
          for (int p = 0; p < parts; ++p) v += part[(p * R + r) * HP + hh];
          sc[k] = v;
        }
      }
      const float mnew = fmaxf(m_run, group_max<32>(fmaxf(sc[0], sc[1])));
      const float alpha = m_run == -INFINITY ? 0.0f : expf(m_run - mnew);
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = hl + 32 * k;
        const float e = r < rows ? expf(sc[k] - mnew) : 0.0f;
        if (r < R) pt[r * HP + hh] = e;
        sum += e;
      }
      l_run = fmaf(l_run, alpha, group_sum<32>(sum));
      m_run = mnew;
      if (hl == 0) alpha_s[hh] = alpha;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < HP; ++h) {
      const float al = alpha_s[h];
#pragma unroll
      for (int c = 0; c < COLS; ++c) acc[h][c] *= al;
    }
    for (int r = 0; r < rows; ++r) {
      float p[HP];
#pragma unroll
      for (int q = 0; q < HP / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(pt + r * HP + 4 * q);
        p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        const int col = t + c * kAttnThreads;
        const float xv = col < dim ? xs[r * S + col] : 0.0f;
#pragma unroll
        for (int h = 0; h < HP; ++h) acc[h][c] = fmaf(p[h], xv, acc[h][c]);
      }
    }
  }
  float *dst = partial + (int64_t)b * heads * dim;      // [chunks][heads][dim], the chunks of a segment consecutive
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int col = t + c * kAttnThreads;
      if (h < heads && col < dim) dst[h * dim + col] = acc[h][c];
    }
  if (hh < heads && hl == 0) {
    stat_partial[(int64_t)b * 2 * heads + hh] = m_run;
    stat_partial[(int64_t)b * 2 * heads + heads + hh] = l_run;
  }
}

// out[g,h,d] = sum_c acc_c[h,d] e^(m_c - M) / sum_c l_c e^(m_c - M) over the chunks c of g in chunk order, M = max_c m_c;
// stats[g] = [M (heads) | M + log L (heads)]; an empty segment pools to 0 with stats 0
__global__ __launch_bounds__(256) void k_attn_merge(const float *__restrict__ partial,
                                                     const float *__restrict__ stat_partial,
                                                     const int32_t *__restrict__ chunk_start, int dim, int heads,
                                                     int64_t segments, float *__restrict__ out, float *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segments * heads * dim) return;
  const int d = (int)(i % dim);
  const int64_t gh = i / dim;
  const int h = (int)(gh % heads);
  const int64_t g = gh / heads;
  const int c0 = chunk_start[g], c1 = chunk_start[g + 1];
  float M = -INFINITY;
  for (int c = c0; c < c1; ++c) M = fmaxf(M, stat_partial[(int64_t)c * 2 * heads + h]);
  float L = 0.0f, acc = 0.0f;
  for (int c = c0; c < c1; ++c) {
    const float w = expf(stat_partial[(int64_t)c * 2 * heads + h] - M);
    L = fmaf(stat_partial[(int64_t)c * 2 * heads + heads + h], w, L);
    acc = fmaf(partial[((int64_t)c * heads + h) * dim + d], w, acc);
  }
  const bool empty = c0 == c1;
  out[i] = empty ? 0.0f : acc / L;
  if (d == 0) {
    stats[g * 2 * heads + h] = empty ? 0.0f : M;
    stats[g * 2 * heads + heads + h] = empty ? 0.0f : M + logf(L);
  }
}

// LDS (floats): xs [R][S] | ut, dpt [dim][HP] | part_s, part_a [256][HP] | pt, dst [R][HP]
template <int HP, int COLS>
__global__ __launch_bounds__(kAttnThreads) void k_attn_pool_backward(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ u, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int heads, int R, int S, int num_segments,
    const int32_t *__restrict__ chunk_start, bool vec4, const float *__restrict__ pooled,
    const float *__restrict__ stats, const float *__restrict__ grad_out, float *__restrict__ grad_x, int64_t ld_gx,
    float *__restrict__ du_partial) {
  extern __shared__ float lds[];
  const int b = blockIdx.x;
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, b, ch)) return;
  const int parts = kAttnThreads / R;
  float *xs = lds;
  float *ut = xs + R * S;
  float *dpt = ut + dim * HP;
  float *part_s = dpt + dim * HP;
  float *part_a = part_s + kAttnThreads * HP;
  float *pt = part_a + kAttnThreads * HP;
  float *dst = pt + R * HP;
  const int t = threadIdx.x;
  const float *useg = u + (int64_t)ch.seg * heads * dim;
  const float *gseg = grad_out + (int64_t)ch.seg * heads * dim;
  attn_stage_heads<HP>(ut, useg, dim, heads);
  attn_stage_heads<HP>(dpt, gseg, dim, heads);
  for (int e = t; e < R * HP; e += kAttnThreads) pt[e] = dst[e] = 0.0f;
  const int hh = t >> 5, hl = t & 31;
  float lse = 0.0f, abar = 0.0f;
  if (hh < heads) {                                     // abar = dP[g,h] . P[g,h], a fixed-order half-wave sum
    const float *pg = pooled + ((int64_t)ch.seg * heads + hh) * dim;
    const float *gg = gseg + (int64_t)hh * dim;
    float v = 0.0f;
    for (int d = hl; d < dim; d += 32) v = fmaf(gg[d], pg[d], v);
    abar = group_sum<32>(v);
    lse = stats[(int64_t)ch.seg * 2 * heads + heads + hh];
  }
  float uc[HP][COLS], gc[HP][COLS], dacc[HP][COLS];     // the thread's columns of u and dP, its du accumulators
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int col = t + c * kAttnThreads;
      const bool in = h < heads && col < dim;
      uc[h][c] = in ? useg[(int64_t)h * dim + col] : 0.0f;
      gc[h][c] = in ? gseg[(int64_t)h * dim + col] : 0.0f;
      dacc[h][c] = 0.0f;
    }
  const int wr = t % R, wp = t / R;
  const int slice = (dim + parts - 1) / parts;
  const int d0 = wp * slice < dim ? wp * slice : dim, d1 = d0 + slice < dim ? d0 + slice : dim;

  for (int t0 = ch.lo; t0 < ch.hi; t0 += R) {
    const int rows = ch.hi - t0 < R ? ch.hi - t0 : R;
    __syncthreads();
    attn_stage_rows(xs, S, x, ld_x, perm, t0, rows, dim, vec4);
    __syncthreads();
    {
      float s[HP], a[HP];
#pragma unroll
      for (int h = 0; h < HP; ++h) s[h] = a[h] = 0.0f;
      if (wr < rows) attn_score_walk<HP, true>(xs + wr * S, ut, dpt, d0, d1, s, a);
#pragma unroll
      for (int q = 0; q < HP / 4; ++q) {
        *reinterpret_cast<float4 *>(part_s + (wp * R + wr) * HP + 4 * q) =
            make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
        *reinterpret_cast<float4 *>(part_a + (wp * R + wr) * HP + 4 * q) =
            make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
      }
    }
    __syncthreads();
    if (hh < heads) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int r = hl + 32 * k;
        if (r < R) {
          float p = 0.0f, ds = 0.0f;
          if (r < rows) {
            float sv = 0.0f, av = 0.0f;
            for (int q = 0; q < parts; ++q) {
              sv += part_s[(q * R + r) * HP + hh];
              av += part_a[(q * R + r) * HP + hh];
            }
            p = expf(sv - lse);
            ds = p * (av - abar);
          }
          pt[r * HP + hh] = p;
          dst[r * HP + hh] = ds;
        }
      }
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      float p[HP], ds[HP];
#pragma unroll
      for (int q = 0; q < HP / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(pt + r * HP + 4 * q);
        const float4 w = *reinterpret_cast<const float4 *>(dst + r * HP + 4 * q);
        p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
        ds[4 * q] = w.x; ds[4 * q + 1] = w.y; ds[4 * q + 2] = w.z; ds[4 * q + 3] = w.w;
      }
      float *gxr = grad_x + (int64_t)perm[t0 + r] * ld_gx;
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        const int col = t + c * kAttnThreads;
        if (col < dim) {
          const float xv = xs[r * S + col];
          float gx = 0.0f;
#pragma unroll
          for (int h = 0; h < HP; ++h) {
            gx = fmaf(p[h], gc[h][c], gx);
            gx = fmaf(ds[h], uc[h][c], gx);
            dacc[h][c] = fmaf(ds[h], xv, dacc[h][c]);
          }
          gxr[col] = gx;
        }
      }
    }
  }
  float *out = du_partial + (int64_t)b * heads * dim;
#pragma unroll
  for (int h = 0; h < HP; ++h)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      const int col = t + c * kAttnThreads;
      if (h < heads && col < dim) out[h * dim + col] = dacc[h][c];
    }
}

// out[g,h,d] = scale * sum_k w[h*dk + k, d] * a[g, h*dk + k]
__global__ __launch_bounds__(256) void k_head_expand(const float *__restrict__ a, const float *__restrict__ w,
                                                      int64_t rows, int heads, int dk, int dim, float scale,
                                                      float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * heads * dim) return;
  const int d = (int)(i % dim);
  const int64_t gh = i / dim;
  const int h = (int)(gh % heads);
  const int64_t g = gh / heads;
  const float *ar = a + g * heads * dk + (int64_t)h * dk;
  const float *wc = w + (int64_t)h * dk * dim + d;
  float v = 0.0f;
  for (int k = 0; k < dk; ++k) v = fmaf(wc[(int64_t)k * dim], ar[k], v);
  out[i] = v * scale;
}

// out[g, j] = scale * sum_d w[j, d] * b[g, j / dk, d]: one wave per (g, j), a fixed-order butterfly over its lanes
__global__ __launch_bounds__(256) void k_head_contract(const float *__restrict__ b, const float *__restrict__ w,
                                                        int64_t rows, int heads, int dk, int dim, float scale,
                                                        float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int hidden = heads * dk;
  if (pair >= rows * hidden) return;                   // uniform per wave
  const int j = (int)(pair % hidden);
  const int64_t g = pair / hidden;
  const float *wr = w + (int64_t)j * dim;
  const float *br = b + (g * heads + j / dk) * dim;
  float v = 0.0f;
  for (int d = lane; d < dim; d += 64) v = fmaf(wr[d], br[d], v);
  v = group_sum(v);
  if (lane == 0) out[pair] = v * scale;
}

// grad_w[j, d] = scale * sum_g a[g, j] * b[g, j / dk, d]   (four interleaved partial sums, added in a fixed order)
__global__ __launch_bounds__(256) void k_head_weight_grad(const float *__restrict__ a, const float *__restrict__ b,
                                                           int64_t rows, int heads, int dk, int dim, float scale,
                                                           float *__restrict__ grad_w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int hidden = heads * dk;
  if (i >= (int64_t)hidden * dim) return;
  const int d = (int)(i % dim);
  const int j = (int)(i / dim);
  const int64_t sa = hidden, sb = (int64_t)heads * dim;
  const float *ap = a + j;
  const float *bp = b + (int64_t)(j / dk) * dim + d;
  float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, v3 = 0.0f;
  int64_t g = 0;
  for (; g + 4 <= rows; g += 4) {
    v0 = fmaf(ap[g * sa], bp[g * sb], v0);
    v1 = fmaf(ap[(g + 1) * sa], bp[(g + 1) * sb], v1);
    v2 = fmaf(ap[(g + 2) * sa], bp[(g + 2) * sb], v2);
    v3 = fmaf(ap[(g + 3) * sa], bp[(g + 3) * sb], v3);
  }
  for (; g < rows; ++g) v0 = fmaf(ap[g * sa], bp[g * sb], v0);
  grad_w[i] = ((v0 + v1) + (v2 + v3)) * scale;
}

template <typename Kern, typename... Args>
int attn_launch(Kern kern, const AttnLayout &L, unsigned grid, hipStream_t st, Args... args) {
  return tile_launch("attention_pool", kern, L.bytes, grid, st, args...);
}

// instantiate KERNEL<HP, COLS> for the layout and launch it
#define ATTN_DISPATCH(RC, KERNEL, L, GRID, ST, ...)                                                      \
  do {                                                                                                    \
    if ((L).HP == 4)                                                                                      \
      RC = (L).cols == 1   ? attn_launch(KERNEL<4, 1>, L, GRID, ST, __VA_ARGS__)                          \
           : (L).cols == 2 ? attn_launch(KERNEL<4, 2>, L, GRID, ST, __VA_ARGS__)                          \
                           : attn_launch(KERNEL<4, 4>, L, GRID, ST, __VA_ARGS__);                         \
    else                                                                                                  \
      RC = (L).cols == 1   ? attn_launch(KERNEL<8, 1>, L, GRID, ST, __VA_ARGS__)                          \
           : (L).cols == 2 ? attn_launch(KERNEL<8, 2>, L, GRID, ST, __VA_ARGS__)                          \
                           : attn_launch(KERNEL<8, 4>, L, GRID, ST, __VA_ARGS__);                         \
  } while (0)

bool attn_supported(int dim, int heads) {
  return heads >= 1 && heads <= kAttnMaxHeads && dim >= 1 && dim <= kAttnMaxDim &&
         attn_layout(dim, heads, true).bytes <= kAttnMaxLds;
}

// forward: the chunk table, the chunks' [heads, dim] accumulators and their (max | sum) per head; backward: the chunk
// table and the chunks' [heads, dim] partial rows of du
struct AttnWorkspace {
  size_t chunk_start, partial, stat_partial, total;
};

AttnWorkspace attn_workspace(int64_t segments, int64_t elements, int dim, int heads, bool backward) {
  const size_t bound = (size_t)chunk_count_bound(segments, elements);
  Carve c;
  AttnWorkspace w;
  w.chunk_start = c.take(chunk_table_bytes(segments));
  w.partial = c.take(bound * heads * dim * sizeof(float));
  w.stat_partial = backward ? 0 : c.take(bound * 2 * heads * sizeof(float));
  w.total = c.off;
  return w;
}

// the argument checks the forward and the backward share; 0 when the arguments are fine
int attn_check(const char *what, int64_t num_segments, int64_t num_elements, int32_t dim, int32_t num_heads) {
  PTGNN_REQUIRE(num_heads > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  if (const int rc = chunked_segments_check(what, num_segments, num_elements, dim)) return rc;
  PTGNN_REQUIRE(num_segments == 0 || attn_supported(dim, num_heads), PTGNN_AMD_EUNSUPPORTED,
                "%s: dim %d / %d heads outside the kernel range (dim <= %d, heads <= %d)", what, dim, num_heads,
                kAttnMaxDim, kAttnMaxHeads);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_attention_pool_supported(int32_t dim, int32_t num_heads) {
  return attn_supported(dim, num_heads) ? 1 : 0;
}

extern "C" size_t ptgnn_amd_attention_pool_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                           int32_t num_heads) {
  if (num_segments <= 0 || dim <= 0 || num_heads <= 0) return 0;
  return attn_workspace(num_segments, num_elements, dim, num_heads, false).total;
}

extern "C" int ptgnn_amd_attention_pool_f32(const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                                            const int32_t *perm, int64_t num_segments, int64_t num_elements,
                                            int32_t dim, int32_t num_heads, float *out, float *stats, void *workspace,
                                            size_t workspace_bytes, void *stream_) {
  if (const int rc = attn_check("attention_pool", num_segments, num_elements, dim, num_heads)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(u && rowptr && out && stats && (num_elements == 0 || (x && perm)), PTGNN_AMD_EINVAL,
                "attention_pool: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || ld_x >= dim, PTGNN_AMD_EINVAL, "attention_pool: bad leading dimension");
  const AttnWorkspace ws = attn_workspace(num_segments, num_elements, dim, num_heads, false);
  if (const int rc = workspace_check("attention_pool", workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *partial = carved<float>(workspace, ws.partial);
  float *stat_partial = carved<float>(workspace, ws.stat_partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const AttnLayout L = attn_layout(dim, num_heads, false);
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_x % 4 == 0 && aligned16(x);
  if (bound > 0) {
    int rc = PTGNN_AMD_OK;
    ATTN_DISPATCH(rc, k_attn_pool_partial, L, (unsigned)bound, st, x, ld_x, u, rowptr, perm, (int)dim, (int)num_heads,
                  L.R, L.S, (int)num_segments, (const int32_t *)chunk_start, vec4, partial, stat_partial);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  const int64_t total = num_segments * num_heads * dim;
  k_attn_merge<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(partial, stat_partial, chunk_start, dim, num_heads,
                                                                 num_segments, out, stats);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_ATTENTION_POOL);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_attention_pool_backward_workspace_bytes(int64_t num_segments, int64_t num_elements,
                                                                    int32_t dim, int32_t num_heads) {
  if (num_segments <= 0 || dim <= 0 || num_heads <= 0) return 0;
  return attn_workspace(num_segments, num_elements, dim, num_heads, true).total;
}

extern "C" int ptgnn_amd_attention_pool_backward_f32(const float *x, int64_t ld_x, const float *u,
                                                     const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                                     int64_t num_elements, int32_t dim, int32_t num_heads,
                                                     const float *pooled, const float *stats, const float *grad_out,
                                                     float *grad_x, int64_t ld_gx, float *grad_u, void *workspace,
                                                     size_t workspace_bytes, void *stream_) {
  if (const int rc = attn_check("attention_pool_backward", num_segments, num_elements, dim, num_heads)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(u && rowptr && pooled && stats && grad_out && grad_u && (num_elements == 0 || (x && perm && grad_x)),
                PTGNN_AMD_EINVAL, "attention_pool_backward: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || (ld_x >= dim && ld_gx >= dim), PTGNN_AMD_EINVAL,
                "attention_pool_backward: bad leading dimension");
  const AttnWorkspace ws = attn_workspace(num_segments, num_elements, dim, num_heads, true);
  if (const int rc = workspace_check("attention_pool_backward", workspace, workspace_bytes, ws.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  float *partial = carved<float>(workspace, ws.partial);
  launch_chunk_starts(rowptr, (int)num_segments, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  const AttnLayout L = attn_layout(dim, num_heads, true);
  const bool vec4 = num_elements > 0 && dim % 4 == 0 && ld_x % 4 == 0 && aligned16(x);
  if (bound > 0) {
    int rc = PTGNN_AMD_OK;
    ATTN_DISPATCH(rc, k_attn_pool_backward, L, (unsigned)bound, st, x, ld_x, u, rowptr, perm, (int)dim, (int)num_heads,
                  L.R, L.S, (int)num_segments, (const int32_t *)chunk_start, vec4, pooled, stats, grad_out, grad_x,
                  ld_gx, partial);
    if (rc != PTGNN_AMD_OK) return rc;
  }
  launch_fold_segments(partial, chunk_start, num_heads * dim, num_segments, grad_u, (int64_t)num_heads * dim, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_ATTENTION_POOL_BACKWARD);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_head_projection_f32(int mode, const float *a, const float *b, const float *w,
                                             int64_t num_rows, int32_t num_heads, int32_t head_dim, int32_t dim,
                                             float scale, float *out, void *stream_) {
  PTGNN_REQUIRE(mode >= 0 && mode <= 2 && num_rows >= 0 && num_heads > 0 && head_dim > 0 && dim > 0, PTGNN_AMD_EINVAL,
                "head_projection: bad mode / sizes");
  hipStream_t st = (hipStream_t)stream_;
  const int64_t hidden = (int64_t)num_heads * head_dim;
  if (mode == 0) {                                      // expand: out [rows, heads, dim] from a [rows, hidden] and w
    if (num_rows == 0) return PTGNN_AMD_OK;
    PTGNN_REQUIRE(a && w && out, PTGNN_AMD_EINVAL, "head_projection: null pointer");
    const int64_t total = num_rows * num_heads * dim;
    k_head_expand<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a, w, num_rows, num_heads, head_dim, dim, scale, out);
  } else if (mode == 1) {                               // contract: out [rows, hidden] from b [rows, heads, dim] and w
    if (num_rows == 0) return PTGNN_AMD_OK;
    PTGNN_REQUIRE(b && w && out, PTGNN_AMD_EINVAL, "head_projection: null pointer");
    const int64_t threads = num_rows * hidden * 64;
    k_head_contract<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(b, w, num_rows, num_heads, head_dim, dim, scale,
                                                                        out);
  } else {                                              // weight gradient: out [hidden, dim] from a and b
    PTGNN_REQUIRE(out && (num_rows == 0 || (a && b)), PTGNN_AMD_EINVAL, "head_projection: null pointer");
    const int64_t total = hidden * dim;
    k_head_weight_grad<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a, b, num_rows, num_heads, head_dim, dim,
                                                                         scale, out);
  }
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_HEAD_PROJECTION);
  return PTGNN_AMD_OK;
}
