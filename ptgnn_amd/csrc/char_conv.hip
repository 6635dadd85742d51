// The char-CNN of CharUnitEmbedder (embeddings/strelementrepresentationmodel.py:128-142) around the windowed GEMMs
// (ptgnn_amd_window_linear_f32 / _window_weight_grad_f32, dense_f32.hip / edge_wgrad.hip):
//   ptgnn_amd_char_embed_f32           the first convolution over the one-hot input as a table sum (no [B, L, C] tensor)
//   ptgnn_amd_char_embed_backward_f32  its table / bias gradient: per-chunk LDS accumulation, folded in chunk order
//   ptgnn_amd_window_max_f32           max over the valid rows of every sample's row frame, lowest position on a tie
//   ptgnn_amd_window_max_backward_f32  the gradient frame of that max: the winner row per (sample, column), zeros elsewhere
// Contracts + reference lines: include/ptgnn_amd.h.
#include "common.h"

namespace ptgnn_amd {
namespace {

constexpr int kCharMaxDim = 1024;
constexpr int kCharMaxWindow = 16;
constexpr int kCharBwdCols = 64;          // columns of a backward tile = lanes of its one wave
constexpr int kCharBwdChunk = 256;        // samples per backward chunk (ptgnn_amd_char_embed_backward_chunk)
constexpr size_t kCharMaxLds = 160 * 1024;   // LDS of one CU (gfx950)

__device__ __forceinline__ int clamp_id(int64_t id, int num_chars) {
  return id < 0 ? 0 : (id >= num_chars ? num_chars - 1 : (int)id);
}

// a1[b R + p, :] = act(bias + sum_k table[k C + chars[b, p + k], :]); one thread per 4 columns of one output row
template <bool RELU>
__global__ __launch_bounds__(256) void k_char_embed(const int64_t *__restrict__ chars, int64_t num_rows, int L, int C,
                                                    int W, int R, const float *__restrict__ table,
                                                    const float *__restrict__ bias, int dim, float *__restrict__ out,
                                                    int64_t ld_out) {
  const int q = dim / 4;
  const int64_t total = num_rows * q;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int64_t b = r / R;
    const int p = (int)(r - b * R);
    const int64_t *cp = chars + b * L + p;
    float4 acc = bias ? *reinterpret_cast<const float4 *>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < W; ++k) {
      const int id = clamp_id(cp[k], C);
      const float4 t = *reinterpret_cast<const float4 *>(table + ((int64_t)k * C + id) * dim + c);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    if (RELU) {
      acc.x = acc.x > 0.f ? acc.x : 0.f;
      acc.y = acc.y > 0.f ? acc.y : 0.f;
      acc.z = acc.z > 0.f ? acc.z : 0.f;
      acc.w = acc.w > 0.f ? acc.w : 0.f;
    }
    *reinterpret_cast<float4 *>(out + r * ld_out + c) = acc;
  }
}

// One wave per (chunk of samples, 64-column tile): lane l owns column l of an LDS copy of the table tile plus one row for
// the bias, and adds the masked gradient rows of its chunk into it in row order -- no lane ever touches another lane's
// column, so there is neither a barrier nor an atomic, and the sum of a chunk has one order.  8 rows are loaded ahead of
// their LDS updates.
template <bool RELU>
__global__ __launch_bounds__(kCharBwdCols) void k_char_embed_backward_partial(
    const float *__restrict__ g, int64_t ld_g, const float *__restrict__ a1, int64_t ld_a,
    const int64_t *__restrict__ chars, int64_t B, int L, int C, int W, int R, int dim, float *__restrict__ partial) {
  extern __shared__ float tile[];
  const int lane = threadIdx.x;
  const int trows = W * C + 1;
  for (int i = 0; i < trows; ++i) tile[i * kCharBwdCols + lane] = 0.f;
  const int col = blockIdx.y * kCharBwdCols + lane;
  const bool live = col < dim;
  const int colc = live ? col : dim - 1;
  const int64_t b0 = (int64_t)blockIdx.x * kCharBwdChunk;
  const int64_t b1 = b0 + kCharBwdChunk < B ? b0 + kCharBwdChunk : B;
  const int64_t r0 = b0 * R, r1 = b1 * R;
  int64_t b = b0;
  int p = 0;
  constexpr int U = 8;
  float *const brow = tile + (trows - 1) * kCharBwdCols + lane;
  for (int64_t r = r0; r < r1; r += U) {
    float gv[U], av[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r + u < r1 ? r + u : r1 - 1;
      gv[u] = g[rr * ld_g + colc];
      av[u] = RELU ? a1[rr * ld_a + colc] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r + u < r1) {
        const float m = av[u] > 0.f ? gv[u] : 0.f;
        const int64_t *cp = chars + b * L + p;
        for (int k = 0; k < W; ++k) tile[(k * C + clamp_id(cp[k], C)) * kCharBwdCols + lane] += m;
        *brow += m;
        if (++p == R) { p = 0; ++b; }
      }
    }
  }
  if (live) {
    float *dst = partial + (int64_t)blockIdx.x * trows * dim + col;
    for (int i = 0; i < trows; ++i) dst[(int64_t)i * dim] = tile[i * kCharBwdCols + lane];
  }
}

// grad_table / grad_bias = the chunks' partial tiles added in chunk order; one thread per element
__global__ __launch_bounds__(256) void k_char_embed_backward_fold(const float *__restrict__ partial, int64_t chunks,
                                                                  int table_rows, int dim,
                                                                  float *__restrict__ grad_table,
                                                                  float *__restrict__ grad_bias) {
  const int64_t per = (int64_t)(table_rows + 1) * dim;
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= per) return;
  float acc = 0.f;
  for (int64_t c = 0; c < chunks; ++c) acc += partial[c * per + i];
  if (i < (int64_t)table_rows * dim) grad_table[i] = acc;
  else if (grad_bias) grad_bias[i - (int64_t)table_rows * dim] = acc;
}

// torch.max(dim): the first position that attains the maximum; a NaN wins from where it first appears
template <int VEC>
__global__ __launch_bounds__(256) void k_window_max(const float *__restrict__ x, int64_t ld_x, int64_t B, int R,
                                                    int valid, int dim, float *__restrict__ out, int64_t ld_out,
                                                    int32_t *__restrict__ arg) {
  const int q = dim / VEC;
  const int64_t total = B * q;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / q;
    const int c = (int)(i - b * q) * VEC;
    const float *src = x + b * R * ld_x + c;
    float best[VEC];
    int at[VEC];
    vec_load<VEC>(src, best);
#pragma unroll
    for (int j = 0; j < VEC; ++j) at[j] = 0;
    for (int p = 1; p < valid; ++p) {
      float v[VEC];
      vec_load<VEC>(src + (int64_t)p * ld_x, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const bool take = best[j] == best[j] && (v[j] > best[j] || v[j] != v[j]);
        best[j] = take ? v[j] : best[j];
        at[j] = take ? p : at[j];
      }
    }
    vec_store<VEC>(out + b * ld_out + c, best);
    if (arg) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) arg[b * dim + c + j] = at[j];
    }
  }
}

// every row of the [B R, dim] gradient frame: grad[b, d] at row arg[b, d] of sample b, exact zeros elsewhere
template <int VEC>
__global__ __launch_bounds__(256) void k_window_max_backward(const float *__restrict__ g, int64_t ld_g,
                                                             const int32_t *__restrict__ arg, int64_t num_rows, int R,
                                                             int dim, float *__restrict__ gx, int64_t ld_gx) {
  const int q = dim / VEC;
  const int64_t total = num_rows * q;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / q;
    const int c = (int)(i - r * q) * VEC;
    const int64_t b = r / R;
    const int p = (int)(r - b * R);
    float gv[VEC], o[VEC];
    vec_load<VEC>(g + b * ld_g + c, gv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = arg[b * dim + c + j] == p ? gv[j] : 0.f;
    vec_store<VEC>(gx + r * ld_gx + c, o);
  }
}

inline unsigned grid_for(int64_t items) {
  int64_t blocks = (items + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

inline size_t char_bwd_lds(int num_chars, int window) {
  return (size_t)(window * num_chars + 1) * kCharBwdCols * sizeof(float);
}

inline int64_t char_bwd_chunks(int64_t num_samples) { return (num_samples + kCharBwdChunk - 1) / kCharBwdChunk; }

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_char_embed_supported(int32_t num_chars, int32_t window, int32_t dim) {
  if (num_chars < 1 || window < 1 || window > kCharMaxWindow || dim < 4 || dim > kCharMaxDim || dim % 4 != 0) return 0;
  if ((int64_t)num_chars * window > (int64_t)1 << 20) return 0;
  return char_bwd_lds(num_chars, window) <= kCharMaxLds ? 1 : 0;   // the backward's table tile must fit one CU's LDS
}

extern "C" int32_t ptgnn_amd_char_embed_backward_chunk(void) { return kCharBwdChunk; }

extern "C" int ptgnn_amd_char_embed_f32(const int64_t *chars, int64_t num_samples, int32_t length, int32_t num_chars,
                                        int32_t window, const float *table, const float *bias, int32_t dim, int act,
                                        float *out, int64_t ld_out, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && length > 0 && num_chars > 0 && window > 0 && dim > 0 && window <= length,
                PTGNN_AMD_EINVAL, "char_embed: bad sizes");
  PTGNN_REQUIRE(act == PTGNN_AMD_ACT_NONE || act == PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "char_embed: bad act");
  PTGNN_REQUIRE(ptgnn_amd_char_embed_supported(num_chars, window, dim), PTGNN_AMD_EUNSUPPORTED,
                "char_embed: num_chars=%d window=%d dim=%d is outside the kernel range", num_chars, window, dim);
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(chars && table && out && ld_out >= dim, PTGNN_AMD_EINVAL, "char_embed: null/ld");
  PTGNN_REQUIRE(ld_out % 4 == 0 && aligned16(table) && aligned16(out) && (!bias || aligned16(bias)),
                PTGNN_AMD_EUNSUPPORTED, "char_embed: rows must be 16-byte aligned");
  const int R = length - window + 1;
  const int64_t num_rows = num_samples * R;
  hipStream_t st = (hipStream_t)stream_;
  const unsigned grid = grid_for(num_rows * (dim / 4));
  if (act == PTGNN_AMD_ACT_RELU)
    k_char_embed<true><<<grid, 256, 0, st>>>(chars, num_rows, length, num_chars, window, R, table, bias, dim, out, ld_out);
  else
    k_char_embed<false><<<grid, 256, 0, st>>>(chars, num_rows, length, num_chars, window, R, table, bias, dim, out, ld_out);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_CHAR_EMBED);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_char_embed_backward_workspace_bytes(int64_t num_samples, int32_t num_chars, int32_t window,
                                                                int32_t dim) {
  if (num_samples <= 0 || num_chars <= 0 || window <= 0 || dim <= 0) return 0;
  return (size_t)char_bwd_chunks(num_samples) * (size_t)(window * num_chars + 1) * (size_t)dim * sizeof(float);
}

extern "C" int ptgnn_amd_char_embed_backward_f32(const float *grad, int64_t ld_grad, const float *a1, int64_t ld_a1,
                                                 const int64_t *chars, int64_t num_samples, int32_t length,
                                                 int32_t num_chars, int32_t window, int32_t dim, int act,
                                                 float *grad_table, float *grad_bias, void *workspace,
                                                 size_t workspace_bytes, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && length > 0 && num_chars > 0 && window > 0 && dim > 0 && window <= length,
                PTGNN_AMD_EINVAL, "char_embed_backward: bad sizes");
  PTGNN_REQUIRE(act == PTGNN_AMD_ACT_NONE || act == PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "char_embed_backward: bad act");
  PTGNN_REQUIRE(ptgnn_amd_char_embed_supported(num_chars, window, dim), PTGNN_AMD_EUNSUPPORTED,
                "char_embed_backward: num_chars=%d window=%d dim=%d is outside the kernel range", num_chars, window, dim);
  PTGNN_REQUIRE(grad_table, PTGNN_AMD_EINVAL, "char_embed_backward: null pointer");
  hipStream_t st = (hipStream_t)stream_;
  const int table_rows = window * num_chars;
  if (num_samples == 0) {
    PTGNN_HIP(hipMemsetAsync(grad_table, 0, sizeof(float) * (size_t)table_rows * dim, st));
    if (grad_bias) PTGNN_HIP(hipMemsetAsync(grad_bias, 0, sizeof(float) * dim, st));
    return PTGNN_AMD_OK;
  }
  const bool relu = act == PTGNN_AMD_ACT_RELU;
  PTGNN_REQUIRE(grad && chars && (a1 || !relu) && ld_grad >= dim && (!relu || ld_a1 >= dim), PTGNN_AMD_EINVAL,
                "char_embed_backward: null pointer / ld");
  PTGNN_REQUIRE(workspace && workspace_bytes >= ptgnn_amd_char_embed_backward_workspace_bytes(num_samples, num_chars,
                                                                                              window, dim),
                PTGNN_AMD_EWORKSPACE, "char_embed_backward: workspace too small (%zu bytes)", workspace_bytes);
  const int R = length - window + 1;
  const int64_t chunks = char_bwd_chunks(num_samples);
  PTGNN_REQUIRE(chunks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "char_embed_backward: too many chunks");
  const size_t lds = char_bwd_lds(num_chars, window);
  const dim3 grid((unsigned)chunks, (unsigned)((dim + kCharBwdCols - 1) / kCharBwdCols));
  float *const partial = (float *)workspace;
#define PTGNN_CHAR_BWD(RELU)                                                                                         \
  do {                                                                                                               \
    auto kern = k_char_embed_backward_partial<RELU>;                                                                 \
    PTGNN_REQUIRE(lds <= 64 * 1024 || raise_dynamic_lds(kern, lds), PTGNN_AMD_EHIP,                                  \
                  "char_embed_backward: %zu B of LDS refused", lds);                                                 \
    kern<<<grid, kCharBwdCols, lds, st>>>(grad, ld_grad, a1, ld_a1, chars, num_samples, length, num_chars, window, R, \
                                          dim, partial);                                                             \
  } while (0)
  if (relu) PTGNN_CHAR_BWD(true);
  else PTGNN_CHAR_BWD(false);
#undef PTGNN_CHAR_BWD
  PTGNN_LAUNCH_CHECK();
  const int64_t outs = (int64_t)(table_rows + 1) * dim;
  k_char_embed_backward_fold<<<(unsigned)((outs + 255) / 256), 256, 0, st>>>(partial, chunks, table_rows, dim,
                                                                            grad_table, grad_bias);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_CHAR_EMBED_BACKWARD);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_window_max_f32(const float *x, int64_t ld_x, int64_t num_samples, int32_t rows_per_sample,
                                        int32_t valid, int32_t dim, float *out, int64_t ld_out, int32_t *arg,
                                        void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && rows_per_sample > 0 && dim > 0, PTGNN_AMD_EINVAL, "window_max: bad sizes");
  PTGNN_REQUIRE(valid >= 1 && valid <= rows_per_sample, PTGNN_AMD_EINVAL,
                "window_max: valid=%d is not in [1, rows_per_sample=%d]", valid, rows_per_sample);
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && out && ld_x >= dim && ld_out >= dim, PTGNN_AMD_EINVAL, "window_max: null/ld");
  hipStream_t st = (hipStream_t)stream_;
  const bool v4 = dim % 4 == 0 && ld_x % 4 == 0 && ld_out % 4 == 0 && aligned16(x) && aligned16(out);
  if (v4)
    k_window_max<4><<<grid_for(num_samples * (dim / 4)), 256, 0, st>>>(x, ld_x, num_samples, rows_per_sample, valid, dim,
                                                                        out, ld_out, arg);
  else
    k_window_max<1><<<grid_for(num_samples * dim), 256, 0, st>>>(x, ld_x, num_samples, rows_per_sample, valid, dim, out,
                                                                  ld_out, arg);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_WINDOW_MAX);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_window_max_backward_f32(const float *grad, int64_t ld_grad, const int32_t *arg,
                                                 int64_t num_samples, int32_t rows_per_sample, int32_t dim,
                                                 float *grad_x, int64_t ld_gx, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && rows_per_sample > 0 && dim > 0, PTGNN_AMD_EINVAL, "window_max_backward: bad sizes");
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(grad && arg && grad_x && ld_grad >= dim && ld_gx >= dim, PTGNN_AMD_EINVAL,
                "window_max_backward: null/ld");
  hipStream_t st = (hipStream_t)stream_;
  const int64_t num_rows = num_samples * rows_per_sample;
  const bool v4 = dim % 4 == 0 && ld_grad % 4 == 0 && ld_gx % 4 == 0 && aligned16(grad) && aligned16(grad_x);
  if (v4)
    k_window_max_backward<4><<<grid_for(num_rows * (dim / 4)), 256, 0, st>>>(grad, ld_grad, arg, num_rows,
                                                                              rows_per_sample, dim, grad_x, ld_gx);
  else
    k_window_max_backward<1><<<grid_for(num_rows * dim), 256, 0, st>>>(grad, ld_grad, arg, num_rows, rows_per_sample,
                                                                        dim, grad_x, ld_gx);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_WINDOW_MAX_BACKWARD);
  return PTGNN_AMD_OK;
}
