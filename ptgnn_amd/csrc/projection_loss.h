// What projection_loss.hip (exact fp32) and projection_loss16.hip (16-bit matrix-core inputs) share: the sizes that
// decide who owns what -- and with them both workspace layouts and the fixed fold orders --, the softmax term of G, the
// push of a lane's 16 scores into its running state, the argument checks, and the last launch of the backward.  One copy,
// so the two routes cut a problem into workgroups alike and hand k_vocab_loss_merge and k_projection_loss_fold the same
// layouts.
#pragma once
#include <math.h>

#include "dense_common.h"
#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {

constexpr int kPlThreads = 256;
constexpr int kPlRows = 64;          // rows of p of a workgroup (forward, dproj) / of a step (dtable)
constexpr int kPlStep = 64;          // rows of T of a step (forward, dproj) / of a workgroup (dtable)
constexpr int kPlFwdCols = 256;      // columns of a forward workgroup = of one (max, sum) partial
constexpr int kPlBwdCols = 1024;     // columns of a dproj workgroup = of one partial of d_p
constexpr int kPlMaxDim = 256;
static_assert(kPlFwdCols % kPlStep == 0 && kPlBwdCols % kPlStep == 0, "a chunk is whole steps");

// exp((s - M) - log_sum): the softmax term of G.  An empty state (M = -inf) has none; rows past the end carry M = +inf.
__device__ __forceinline__ float pl_prob(float s, float m, float log_sum) {
  return m == -INFINITY ? 0.0f : expf((s - m) - log_sum);
}

// the 16 scores of a lane into its running state: one rescale for their maximum, their terms added in register order
__device__ __forceinline__ void push_tile(MaxSum &a, const f32x16 &x) {
  float gm = x[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) gm = fmaxf(gm, x[j]);
  if (gm > a.m) {
    a.s = a.m == -INFINITY ? 0.0f : a.s * expf(a.m - gm);
    a.m = gm;
  }
  if (a.m == -INFINITY) return;
  float t = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) t += expf(x[j] - a.m);
  a.s += t;
}

// d_p[r, e] = the column chunks' partials part[chunk, r, e] added in chunk order (k_projection_loss_fold, defined in
// projection_loss.hip)
void launch_projection_loss_fold(const float *part, int64_t rows, int dim, int chunks, float *d_p, int64_t ld_dp,
                                 hipStream_t st);

inline int64_t pl_row_blocks(int64_t rows) { return (rows + kPlRows - 1) / kPlRows; }
inline int64_t pl_fwd_chunks(int32_t vocab) { return ((int64_t)vocab + kPlFwdCols - 1) / kPlFwdCols; }
inline int64_t pl_bwd_chunks(int32_t vocab) { return ((int64_t)vocab + kPlBwdCols - 1) / kPlBwdCols; }

struct PlFwdWs {
  size_t partial, target_score, bytes;
};

inline PlFwdWs pl_fwd_workspace(int64_t rows, int32_t vocab) {
  Carve c;
  PlFwdWs w;
  w.partial = c.take((size_t)rows * pl_fwd_chunks(vocab) * sizeof(float2));
  w.target_score = c.take((size_t)rows * sizeof(float));
  w.bytes = c.off;
  return w;
}

inline size_t pl_bwd_workspace(int64_t rows, int32_t vocab, int32_t dim) {
  Carve c;
  c.take((size_t)pl_bwd_chunks(vocab) * rows * dim * sizeof(float));
  return c.off;
}

// what the entries share: sizes, leading dimensions, and everything a kernel indexes with an int fits one
inline int pl_check(const char *what, const void *p, int64_t ld_p, const void *T, int64_t ld_t, int64_t rows, int32_t vocab,
                    int32_t dim) {
  PTGNN_REQUIRE(rows >= 0 && vocab >= 1 && dim >= 1, PTGNN_AMD_EINVAL, "%s: bad sizes (rows %lld, vocab %d, dim %d)", what,
                (long long)rows, vocab, dim);
  PTGNN_REQUIRE(dim <= kPlMaxDim, PTGNN_AMD_EUNSUPPORTED, "%s: dimension %d exceeds %d", what, dim, kPlMaxDim);
  PTGNN_REQUIRE(ld_p >= dim && ld_t >= dim, PTGNN_AMD_EINVAL, "%s: leading dimension (%lld, %lld) < dim %d", what,
                (long long)ld_p, (long long)ld_t, dim);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(vocab <= lim - 2 * kPlBwdCols && rows <= lim - 2 * kPlRows &&
                    pl_row_blocks(rows) <= (lim - 1) / pl_fwd_chunks(vocab),
                PTGNN_AMD_EUNSUPPORTED, "%s: too many rows / columns", what);
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(p && T, PTGNN_AMD_EINVAL, "%s: null pointer", what);
  return PTGNN_AMD_OK;
}

#define PL_TILES(n, ...)                                   \
  switch (n) {                                             \
    case 1: { constexpr int TT = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int TT = 2; __VA_ARGS__; } break;  \
    case 3: { constexpr int TT = 3; __VA_ARGS__; } break;  \
    case 4: { constexpr int TT = 4; __VA_ARGS__; } break;  \
    case 5: { constexpr int TT = 5; __VA_ARGS__; } break;  \
    case 6: { constexpr int TT = 6; __VA_ARGS__; } break;  \
    case 7: { constexpr int TT = 7; __VA_ARGS__; } break;  \
    default: { constexpr int TT = 8; __VA_ARGS__; } break; \
  }

}  // namespace ptgnn_amd
