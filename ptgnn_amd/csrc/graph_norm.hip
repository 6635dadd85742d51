// GraphNorm (ptgnn/neuralmodels/gnn/messagepassing/graphnorm.py:36-46; arXiv:2009.03294), the normalisation placed between
// message-passing layers: per graph g with n_g nodes, per column, fp32
//
//     mu[g]   = (1 / n_g) sum_{i in g} x_i                        scatter_mean over node_to_graph_idx
//     s_i     = x_i - alpha * mu[g]                                the broadcast mean[idx], materialised [N, D]
//     sig2[g] = (1 / n_g) sum_{i in g} s_i * s_i + eps            pow, the second scatter_mean
//     y_i     = gamma * s_i / sqrt(sig2[g]) + bias                sigma_2[idx], sqrt, div, mul, add: all [N, D]
//
// The reference runs two segment means and about ten elementwise operators -- a dozen passes over [N, D] forward, twice
// that with autograd.  Here the forward is three reads of x and one write of y, the backward two reads of (x, grad_y)
// and one write of grad_x: HBM-bound streaming work whose re-reads fit the Infinity Cache at the benchmarked sizes
// (116 k x 64 fp32 = 30 MB).
//
// Segments are graphs: few and long.  Every segment is cut into the 128-row chunks of segment_chunks.h, counted from its
// own start (chunk_locate and the chunk table are that header's, as for the pools), workgroup b folds chunk c of segment
// g, and a per-graph launch adds the chunk partials of a segment IN CHUNK ORDER (chunk_fold).  No float atomics: a graph's
// statistics and output rows are a fixed function of ITS rows and their order, wherever the graph sits in the batch.
//
// The variance is the reference's two-pass one over the ROUNDED s_i (not var + (1 - alpha)^2 mu^2, which loses y on
// inputs whose mean dwarfs their spread), and every kernel forms s_i the same way: one rounded product alpha * mu[g],
// one rounded subtraction.
//
// Backward, with r = 1 / sqrt(sig2), gy = dL/dy:
//     A[g] = sum gy_i              B[g] = sum gy_i s_i             C[g] = sum s_i
//     c[g] = -gamma B r^3 / n_g    S[g] = gamma r A + c C
//     dx_i = gamma r gy_i + c s_i - (alpha / n_g) S
//     dgamma = sum_g B r           dalpha = -sum_g mu S            dbias = sum_g A
// C is the sum of the rounded s_i (not n (1 - alpha) mu): the cancellation 1 - s^2 / sig2 of a one- or two-node graph
// only survives if sig2 and C are built from the same s_i.  That cancellation is also why the backward's per-graph
// quantities are FLOAT64: on a one-node graph S = gamma r gy (1 - s^2 r^2) is ~0, and fp32 roundings of B, sig2 or r
// leave gamma gy r * 1e-7 instead -- times mu / |1 - alpha| in dalpha (an all-fp32 backward with saved r and C was
// 2.2e-4 from float64 there, where the fp32 reference was 5.7e-5: profiles/graphnorm_notes.md).  So the forward saves
// only mu (s_i has to be the forward's), and the backward sums A, B, C and Q = sum s_i^2 over (x, gy) with float64
// accumulators (products of two floats are exact there; the pass stays memory-bound) and forms sig2, r, c, S in float64.  One pass over (x, gy) gives the chunk
// partials, a per-graph fold gives c, gamma r, (alpha / n) S and the graph's three parameter-gradient terms, those are
// added in GRAPH ORDER, and one streaming pass writes dx.  All outputs are overwritten and deterministic.
#include "segment_chunks.h"

namespace ptgnn_amd {
namespace {

constexpr int kGnThreads = 256;
constexpr int kGnMaxDim = 1024;

enum { kGnSumX = 0, kGnSumSq = 1, kGnSumGrad = 2 };

// Column sums over the rows of one chunk.  A row is `units` column units (float4 or float) wide; `lanes` (a power of two
// <= 256) threads take one unit each, the workgroup's 256 / lanes row groups take every (256 / lanes)-th row of the
// chunk, and thread (0, g) adds the row groups' sums in group order.  Rows wider than `lanes` units are walked once per
// tile of `lanes` units.  partial[b, k * dim + col], k < NOUT:
//   kGnSumX     float   sum x_i
//   kGnSumSq    float   sum s_i s_i
//   kGnSumGrad  double  sum gy_i | sum gy_i s_i | sum s_i s_i | sum s_i
template <int MODE> struct GnSums { using T = float; static constexpr int kOut = 1; };
template <> struct GnSums<kGnSumGrad> { using T = double; static constexpr int kOut = 4; };

template <int VEC, int MODE>
__global__ __launch_bounds__(kGnThreads) void k_graph_norm_chunk_sums(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ gy, int64_t ld_gy,
    const float *__restrict__ alpha, const float *__restrict__ mean, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, int dim, int lanes, int num_segments, const int32_t *__restrict__ chunk_start,
    typename GnSums<MODE>::T *__restrict__ partial) {
  using T = typename GnSums<MODE>::T;
  constexpr int NOUT = GnSums<MODE>::kOut;
  __shared__ __attribute__((aligned(16))) T lds[NOUT][kGnThreads * VEC];
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, blockIdx.x, ch)) return;
  const int groups = kGnThreads / lanes;
  const int grp = threadIdx.x / lanes, g = threadIdx.x % lanes;
  const int units = dim / VEC;
  T *dst = partial + (int64_t)blockIdx.x * NOUT * dim;
  for (int ubase = 0; ubase < units; ubase += lanes) {
    const int col = (ubase + g) * VEC;
    const bool on = ubase + g < units;
    float am[VEC];
    T acc[NOUT][VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      am[v] = 0.0f;
#pragma unroll
      for (int k = 0; k < NOUT; ++k) acc[k][v] = 0;
    }
    if (on) {
      if constexpr (MODE != kGnSumX) {
        float al[VEC], mu[VEC];
        vec_load<VEC>(alpha + col, al);
        vec_load<VEC>(mean + (int64_t)ch.seg * dim + col, mu);
#pragma unroll
        for (int v = 0; v < VEC; ++v) am[v] = __fmul_rn(al[v], mu[v]);
      }
      for (int p = ch.lo + grp; p < ch.hi; p += groups) {
        const int64_t r = perm[p];
        float xv[VEC];
        vec_load<VEC>(x + r * ld_x + col, xv);
        if constexpr (MODE == kGnSumX) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[0][v] += xv[v];
        } else if constexpr (MODE == kGnSumSq) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float s = __fsub_rn(xv[v], am[v]);
            acc[0][v] = fmaf(s, s, acc[0][v]);
          }
        } else {
          float gv[VEC];
          vec_load<VEC>(gy + r * ld_gy + col, gv);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const double s = (double)__fsub_rn(xv[v], am[v]), gd = (double)gv[v];
            acc[0][v] += gd;
            acc[1][v] = fma(gd, s, acc[1][v]);
            acc[2][v] = fma(s, s, acc[2][v]);
            acc[3][v] += s;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NOUT; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) lds[k][threadIdx.x * VEC + v] = acc[k][v];
    __syncthreads();
    if (grp == 0 && on) {
#pragma unroll
      for (int k = 0; k < NOUT; ++k) {
        T t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = 0;
        for (int r = 0; r < groups; ++r)                                   // fixed order
#pragma unroll
          for (int v = 0; v < VEC; ++v) t[v] += lds[k][(r * lanes + g) * VEC + v];
#pragma unroll
        for (int v = 0; v < VEC; ++v) dst[k * dim + col + v] = t[v];
      }
    }
    __syncthreads();
  }
}

// mean[g, :] = mu[g]: the chunk sums of x in chunk order over n_g (0 for a graph without nodes, as scatter_mean)
__global__ __launch_bounds__(256) void k_graph_norm_fold_mean(const float *__restrict__ partial,
                                                               const int32_t *__restrict__ chunk_start,
                                                               const int32_t *__restrict__ rowptr, int dim,
                                                               int64_t segments, float *__restrict__ mean) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segments * dim) return;
  const int64_t g = i / dim;
  const int col = (int)(i % dim);
  const int n = rowptr[g + 1] - rowptr[g];
  const float t = chunk_fold(partial + col, dim, chunk_start[g], chunk_start[g + 1]);
  mean[g * dim + col] = n > 0 ? t / (float)n : 0.0f;
}

// rinv[g, :] = 1 / sqrt(sig2[g])
__global__ __launch_bounds__(256) void k_graph_norm_fold_var(const float *__restrict__ partial,
                                                              const int32_t *__restrict__ chunk_start,
                                                              const int32_t *__restrict__ rowptr, int dim,
                                                              int64_t segments, float eps, float *__restrict__ rinv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segments * dim) return;
  const int64_t g = i / dim;
  const int col = (int)(i % dim);
  const int n = rowptr[g + 1] - rowptr[g];
  const float sq = chunk_fold(partial + col, dim, chunk_start[g], chunk_start[g + 1]);
  const float sig2 = __fadd_rn(sq / (float)(n > 0 ? n : 1), eps);
  rinv[g * dim + col] = 1.0f / sqrtf(sig2);
}

// y_i = gamma r s_i + bias over the rows of one chunk (thread layout of k_graph_norm_chunk_sums)
template <int VEC>
__global__ __launch_bounds__(kGnThreads) void k_graph_norm_apply(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ gamma, const float *__restrict__ alpha,
    const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ rinv,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ perm, int dim, int lanes, int num_segments,
    const int32_t *__restrict__ chunk_start, float *__restrict__ y, int64_t ld_y) {
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, blockIdx.x, ch)) return;
  const int groups = kGnThreads / lanes;
  const int grp = threadIdx.x / lanes, g = threadIdx.x % lanes;
  const int units = dim / VEC;
  const float *mu_g = mean + (int64_t)ch.seg * dim, *r_g = rinv + (int64_t)ch.seg * dim;
  for (int ubase = g; ubase < units; ubase += lanes) {
    const int col = ubase * VEC;
    float ga[VEC], al[VEC], bi[VEC], mu[VEC], r[VEC], am[VEC], gr[VEC];
    vec_load<VEC>(gamma + col, ga);
    vec_load<VEC>(alpha + col, al);
    vec_load<VEC>(bias + col, bi);
    vec_load<VEC>(mu_g + col, mu);
    vec_load<VEC>(r_g + col, r);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      am[v] = __fmul_rn(al[v], mu[v]);
      gr[v] = ga[v] * r[v];
    }
    for (int p = ch.lo + grp; p < ch.hi; p += groups) {
      const int64_t row = perm[p];
      float xv[VEC], o[VEC];
      vec_load<VEC>(x + row * ld_x + col, xv);
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = fmaf(__fsub_rn(xv[v], am[v]), gr[v], bi[v]);
      vec_store<VEC>(y + row * ld_y + col, o);
    }
  }
}

// Per (graph, column), float64: A, B, Q, C folded in chunk order, sig2 = Q / n + eps, r = 1 / sqrt(sig2), then
//   coef[g, 0:dim] = c      coef[g, dim:2dim] = gamma r    coef[g, 2dim:3dim] = (alpha / n) S
//   terms[g, 0:dim] = B r   terms[g, dim:2dim] = -mu S     terms[g, 2dim:3dim] = A      (zeros for a graph without nodes)
__global__ __launch_bounds__(256) void k_graph_norm_backward_fold(
    const double *__restrict__ partial, const int32_t *__restrict__ chunk_start, const int32_t *__restrict__ rowptr,
    const float *__restrict__ gamma, const float *__restrict__ alpha, const float *__restrict__ mean, float eps, int dim,
    int64_t segments, double *__restrict__ coef, double *__restrict__ terms) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segments * dim) return;
  const int64_t g = i / dim;
  const int col = (int)(i % dim);
  const int n = rowptr[g + 1] - rowptr[g];
  double c = 0.0, gr = 0.0, shift = 0.0, tg = 0.0, ta = 0.0, tb = 0.0;
  if (n > 0) {
    const int c0 = chunk_start[g], c1 = chunk_start[g + 1];
    const int64_t stride = 4 * (int64_t)dim;
    const double A = chunk_fold(partial + col, stride, c0, c1);
    const double B = chunk_fold(partial + dim + col, stride, c0, c1);
    const double Q = chunk_fold(partial + 2 * dim + col, stride, c0, c1);
    const double C = chunk_fold(partial + 3 * dim + col, stride, c0, c1);
    const double nd = (double)n, ga = (double)gamma[col], mu = (double)mean[g * dim + col];
    const double sig2 = Q / nd + (double)eps;
    const double r = 1.0 / sqrt(sig2);
    gr = ga * r;
    c = -gr * B / (nd * sig2);
    const double S = gr * (A - B * C / (nd * sig2));
    shift = (double)alpha[col] * S / nd;
    tg = B * r;
    ta = -mu * S;
    tb = A;
  }
  coef[g * 3 * dim + col] = c;
  coef[g * 3 * dim + dim + col] = gr;
  coef[g * 3 * dim + 2 * dim + col] = shift;
  terms[g * 3 * dim + col] = tg;
  terms[g * 3 * dim + dim + col] = ta;
  terms[g * 3 * dim + 2 * dim + col] = tb;
}

// out[0:dim] | out[dim:2dim] | out[2dim:3dim] = the graphs' terms added in graph order
__global__ __launch_bounds__(256) void k_graph_norm_param_fold(const double *__restrict__ terms, int segments, int dim,
                                                                float *__restrict__ grad_gamma,
                                                                float *__restrict__ grad_alpha,
                                                                float *__restrict__ grad_bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * dim) return;
  const double t = chunk_fold(terms + i, 3 * (int64_t)dim, 0, segments);
  float *out = i < dim ? grad_gamma : (i < 2 * dim ? grad_alpha : grad_bias);
  out[i % dim] = (float)t;
}

// dx_i = gamma r gy_i + c s_i - (alpha / n) S over the rows of one chunk: two float64 FMAs per element, one rounding
template <int VEC>
__global__ __launch_bounds__(kGnThreads) void k_graph_norm_backward_apply(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ gy, int64_t ld_gy,
    const float *__restrict__ alpha, const float *__restrict__ mean, const double *__restrict__ coef,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ perm, int dim, int lanes, int num_segments,
    const int32_t *__restrict__ chunk_start, float *__restrict__ gx, int64_t ld_gx) {
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, blockIdx.x, ch)) return;
  const int groups = kGnThreads / lanes;
  const int grp = threadIdx.x / lanes, g = threadIdx.x % lanes;
  const int units = dim / VEC;
  const float *st = mean + (int64_t)ch.seg * dim;
  const double *cf = coef + (int64_t)ch.seg * 3 * dim;
  for (int ubase = g; ubase < units; ubase += lanes) {
    const int col = ubase * VEC;
    float al[VEC], mu[VEC], am[VEC];
    double c[VEC], gr[VEC], shift[VEC];
    vec_load<VEC>(alpha + col, al);
    vec_load<VEC>(st + col, mu);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      am[v] = __fmul_rn(al[v], mu[v]);
      c[v] = cf[col + v];
      gr[v] = cf[dim + col + v];
      shift[v] = cf[2 * dim + col + v];
    }
    for (int p = ch.lo + grp; p < ch.hi; p += groups) {
      const int64_t row = perm[p];
      float xv[VEC], gv[VEC], o[VEC];
      vec_load<VEC>(x + row * ld_x + col, xv);
      vec_load<VEC>(gy + row * ld_gy + col, gv);
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        o[v] = (float)(fma(c[v], (double)__fsub_rn(xv[v], am[v]), gr[v] * (double)gv[v]) - shift[v]);
      vec_store<VEC>(gx + row * ld_gx + col, o);
    }
  }
}

// lanes of one row: the power of two >= the row's column units, at most the workgroup
int gn_lanes(int dim, bool vec4) {
  const int units = vec4 ? dim / 4 : dim;
  int lanes = 1;
  while (lanes < units && lanes < kGnThreads) lanes <<= 1;
  return lanes;
}

// the chunk table, the chunk partials and the two per-graph tables
struct GnWorkspace {
  size_t chunk_start, partial, a, b, total;
};

// `partial_row`: bytes of one chunk's partial sums per column; `a_row` / `b_row`: bytes per graph and column
GnWorkspace gn_workspace(int64_t segments, int64_t elements, int dim, size_t partial_row, size_t a_row, size_t b_row) {
  Carve c;
  GnWorkspace w;
  w.chunk_start = c.take(chunk_table_bytes(segments));
  w.partial = c.take((size_t)chunk_count_bound(segments, elements) * dim * partial_row);
  w.a = c.take((size_t)segments * dim * a_row);
  w.b = c.take((size_t)segments * dim * b_row);
  w.total = c.take(0);             // rounded up like the blocks in front: the size this op has always asked for
  return w;
}

GnWorkspace gn_forward_workspace(int64_t segments, int64_t elements, int dim) {     // a: 1 / sqrt(sig2), b: the means of
  return gn_workspace(segments, elements, dim, sizeof(float), sizeof(float), sizeof(float));   // a call without `mean`
}

GnWorkspace gn_backward_workspace(int64_t segments, int64_t elements, int dim) {    // a: coef, b: terms
  return gn_workspace(segments, elements, dim, 4 * sizeof(double), 3 * sizeof(double), 3 * sizeof(double));
}

// the argument checks the forward and the backward share; 0 when the arguments are fine
int gn_check(const char *what, int64_t num_segments, int64_t num_elements, int32_t dim) {
  if (const int rc = chunked_segments_check(what, num_segments, num_elements, dim, 3 * (int64_t)dim)) return rc;
  PTGNN_REQUIRE(dim <= kGnMaxDim, PTGNN_AMD_EUNSUPPORTED, "%s: dim %d exceeds %d", what, dim, kGnMaxDim);
  PTGNN_REQUIRE(num_segments > 0 || num_elements == 0, PTGNN_AMD_EINVAL, "%s: elements without segments", what);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_graph_norm_supported(int32_t dim) { return dim >= 1 && dim <= kGnMaxDim ? 1 : 0; }

extern "C" size_t ptgnn_amd_graph_norm_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim) {
  if (num_segments <= 0 || num_elements < 0 || dim <= 0) return 0;
  return gn_forward_workspace(num_segments, num_elements, dim).total;
}

extern "C" int ptgnn_amd_graph_norm_f32(const float *x, int64_t ld_x, const float *gamma, const float *alpha,
                                        const float *bias, float eps, const int32_t *rowptr, const int32_t *perm,
                                        int64_t num_segments, int64_t num_elements, int32_t dim, float *y, int64_t ld_y,
                                        float *mean, void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = gn_check("graph_norm", num_segments, num_elements, dim)) return rc;
  if (num_segments == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(gamma && alpha && bias && rowptr && (num_elements == 0 || (x && perm && y)), PTGNN_AMD_EINVAL,
                "graph_norm: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || (ld_x >= dim && ld_y >= dim), PTGNN_AMD_EINVAL, "graph_norm: bad leading dimension");
  const GnWorkspace w = gn_forward_workspace(num_segments, num_elements, dim);
  if (const int rc = workspace_check("graph_norm", workspace, workspace_bytes, w.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, w.chunk_start);
  float *partial = carved<float>(workspace, w.partial);
  float *rinv = carved<float>(workspace, w.a);
  if (!mean) mean = carved<float>(workspace, w.b);
  const bool vec4 = dim % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) &&
                    aligned16(alpha) && aligned16(bias) && aligned16(mean) && aligned16(workspace);
  const int lanes = gn_lanes(dim, vec4);
  const unsigned grid = (unsigned)bound, fold_grid = (unsigned)((num_segments * dim + 255) / 256);
  const int G = (int)num_segments;
  launch_chunk_starts(rowptr, G, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  if (vec4)
    k_graph_norm_chunk_sums<4, kGnSumX><<<grid, kGnThreads, 0, st>>>(x, ld_x, nullptr, 0, alpha, mean, rowptr, perm, dim,
                                                                     lanes, G, chunk_start, partial);
  else
    k_graph_norm_chunk_sums<1, kGnSumX><<<grid, kGnThreads, 0, st>>>(x, ld_x, nullptr, 0, alpha, mean, rowptr, perm, dim,
                                                                     lanes, G, chunk_start, partial);
  PTGNN_LAUNCH_CHECK();
  k_graph_norm_fold_mean<<<fold_grid, 256, 0, st>>>(partial, chunk_start, rowptr, dim, num_segments, mean);
  PTGNN_LAUNCH_CHECK();
  if (vec4)
    k_graph_norm_chunk_sums<4, kGnSumSq><<<grid, kGnThreads, 0, st>>>(x, ld_x, nullptr, 0, alpha, mean, rowptr, perm, dim,
                                                                      lanes, G, chunk_start, partial);
  else
    k_graph_norm_chunk_sums<1, kGnSumSq><<<grid, kGnThreads, 0, st>>>(x, ld_x, nullptr, 0, alpha, mean, rowptr, perm, dim,
                                                                      lanes, G, chunk_start, partial);
  PTGNN_LAUNCH_CHECK();
  k_graph_norm_fold_var<<<fold_grid, 256, 0, st>>>(partial, chunk_start, rowptr, dim, num_segments, eps, rinv);
  PTGNN_LAUNCH_CHECK();
  if (vec4)
    k_graph_norm_apply<4><<<grid, kGnThreads, 0, st>>>(x, ld_x, gamma, alpha, bias, mean, rinv, rowptr, perm, dim, lanes,
                                                       G, chunk_start, y, ld_y);
  else
    k_graph_norm_apply<1><<<grid, kGnThreads, 0, st>>>(x, ld_x, gamma, alpha, bias, mean, rinv, rowptr, perm, dim, lanes,
                                                       G, chunk_start, y, ld_y);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_GRAPH_NORM);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_graph_norm_backward_workspace_bytes(int64_t num_segments, int64_t num_elements,
                                                                int32_t dim) {
  if (num_segments <= 0 || num_elements < 0 || dim <= 0) return 0;
  return gn_backward_workspace(num_segments, num_elements, dim).total;
}

extern "C" int ptgnn_amd_graph_norm_backward_f32(const float *x, int64_t ld_x, const float *grad_y, int64_t ld_gy,
                                                 const float *gamma, const float *alpha, float eps, const float *mean,
                                                 const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                                 int64_t num_elements, int32_t dim, float *grad_x, int64_t ld_gx,
                                                 float *grad_gamma, float *grad_alpha, float *grad_bias, void *workspace,
                                                 size_t workspace_bytes, void *stream_) {
  if (const int rc = gn_check("graph_norm_backward", num_segments, num_elements, dim)) return rc;
  PTGNN_REQUIRE(grad_gamma && grad_alpha && grad_bias, PTGNN_AMD_EINVAL, "graph_norm_backward: null pointer");
  hipStream_t st = (hipStream_t)stream_;
  if (num_segments == 0) {
    PTGNN_HIP(hipMemsetAsync(grad_gamma, 0, (size_t)dim * sizeof(float), st));
    PTGNN_HIP(hipMemsetAsync(grad_alpha, 0, (size_t)dim * sizeof(float), st));
    PTGNN_HIP(hipMemsetAsync(grad_bias, 0, (size_t)dim * sizeof(float), st));
    return PTGNN_AMD_OK;
  }
  PTGNN_REQUIRE(gamma && alpha && mean && rowptr && (num_elements == 0 || (x && grad_y && perm && grad_x)),
                PTGNN_AMD_EINVAL, "graph_norm_backward: null pointer");
  PTGNN_REQUIRE(num_elements == 0 || (ld_x >= dim && ld_gy >= dim && ld_gx >= dim), PTGNN_AMD_EINVAL,
                "graph_norm_backward: bad leading dimension");
  const GnWorkspace w = gn_backward_workspace(num_segments, num_elements, dim);
  if (const int rc = workspace_check("graph_norm_backward", workspace, workspace_bytes, w.total)) return rc;
  const int64_t bound = chunk_count_bound(num_segments, num_elements);
  int32_t *chunk_start = carved<int32_t>(workspace, w.chunk_start);
  double *partial = carved<double>(workspace, w.partial);
  double *coef = carved<double>(workspace, w.a);
  double *terms = carved<double>(workspace, w.b);
  const bool vec4 = dim % 4 == 0 && ld_x % 4 == 0 && ld_gy % 4 == 0 && ld_gx % 4 == 0 && aligned16(x) &&
                    aligned16(grad_y) && aligned16(grad_x) && aligned16(gamma) && aligned16(alpha) && aligned16(mean) &&
                    aligned16(workspace);
  const int lanes = gn_lanes(dim, vec4);
  const unsigned grid = (unsigned)bound, fold_grid = (unsigned)((num_segments * dim + 255) / 256);
  const int G = (int)num_segments;
  launch_chunk_starts(rowptr, G, chunk_start, st);
  PTGNN_LAUNCH_CHECK();
  if (vec4)
    k_graph_norm_chunk_sums<4, kGnSumGrad><<<grid, kGnThreads, 0, st>>>(x, ld_x, grad_y, ld_gy, alpha, mean, rowptr, perm,
                                                                        dim, lanes, G, chunk_start, partial);
  else
    k_graph_norm_chunk_sums<1, kGnSumGrad><<<grid, kGnThreads, 0, st>>>(x, ld_x, grad_y, ld_gy, alpha, mean, rowptr, perm,
                                                                        dim, lanes, G, chunk_start, partial);
  PTGNN_LAUNCH_CHECK();
  k_graph_norm_backward_fold<<<fold_grid, 256, 0, st>>>(partial, chunk_start, rowptr, gamma, alpha, mean, eps, dim,
                                                        num_segments, coef, terms);
  PTGNN_LAUNCH_CHECK();
  k_graph_norm_param_fold<<<(unsigned)((3 * dim + 255) / 256), 256, 0, st>>>(terms, G, dim, grad_gamma, grad_alpha,
                                                                             grad_bias);
  PTGNN_LAUNCH_CHECK();
  if (vec4)
    k_graph_norm_backward_apply<4><<<grid, kGnThreads, 0, st>>>(x, ld_x, grad_y, ld_gy, alpha, mean, coef, rowptr, perm,
                                                                dim, lanes, G, chunk_start, grad_x, ld_gx);
  else
    k_graph_norm_backward_apply<1><<<grid, kGnThreads, 0, st>>>(x, ld_x, grad_y, ld_gy, alpha, mean, coef, rowptr, perm,
                                                                dim, lanes, G, chunk_start, grad_x, ld_gx);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_GRAPH_NORM_BACKWARD);
  return PTGNN_AMD_OK;
}
