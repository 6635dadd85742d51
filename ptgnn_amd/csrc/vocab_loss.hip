// The loss of the copying decoder (ptgnn/neuralmodels/sequence/grucopydecoder.py:118-135, 171-212) without the
// [B L, V] log-probabilities: with R = B L rows (one per decoding location), scores [R, V] the raw output of the second
// vocabulary Linear and s[r, v] = scores[r, v] + bias[v],
//
//   a. vocab_loss            norm[r]   = logaddexp(log sum_v exp s[r, v], extra[r])        extra = the copy normaliser
//                            picked[r] = s[r, targets[r]] - norm[r]
//   b. vocab_loss_backward   grad_scores[r, v] = (g_norm[r] - g_picked[r]) exp(s[r, v] - norm[r]) + g_picked[r] [v == targets[r]]
//                            grad_extra[r]     = (g_norm[r] - g_picked[r]) exp(extra[r] - norm[r])
//                            grad_bias[v]      = sum_r grad_scores[r, v]
//   c. copy_loss_finish      the [B, L] tail: UNK-with-copy mask, logaddexp of the two correct-action terms, length mask,
//                            per-sample mean, batch mean, and the derivatives of that loss w.r.t. its two inputs
//
// Exact fp32, no float atomics; every result is a fixed function of the shapes.
//
// a. The columns of a row are cut into chunks of kFwdCols; workgroup (r, c) walks chunk c of row r ONCE with a running
//    (max, sum) per thread, merges its threads and its four waves (MaxSum of softmax_state.h, which says how) and leaves
//    (max, sum) in the workspace.  The thread that meets column targets[r] leaves s[r, targets[r]] there as well, so no
//    score is read twice.  k_vocab_loss_merge (a thread per row) folds the chunks IN CHUNK ORDER and adds the copy term.
//    It keeps the normaliser as the pair (maximum M, log of the sum relative to M): norm = M + log_sum is rounded at the
//    magnitude of the logits (an ulp of 1.5e-5 at 140), the pair is not, so picked = (s - M) - log_sum and the
//    backward's exp((s - M) - log_sum) stay accurate to 1e-7 however large the logits are.  Thread t of a workgroup
//    owns the same columns whether the row is read with 16-byte loads or (unaligned rows, the ragged tail) dword loads:
//    the bits do not depend on the alignment.
// b. Workgroup (row block, column chunk): kBwdRows rows x kBwdCols columns, thread t four columns; it walks its rows in
//    row order, writes the gradient and keeps the column sums, which it leaves as the row block's partial of grad_bias --
//    the same pass, no second read of [R, V].  k_vocab_bias_fold adds the partials IN ROW-BLOCK ORDER.
// c. One workgroup.  A thread per sample walks the sample's steps in step order (the reference's arithmetic: the length
//    mask is the product any * mask, not a select); the per-sample values are then added in sample order (thread t the
//    t-th contiguous run, thread 0 the runs in thread order).
//
// Traffic: DESIGN.md, "Vocabulary loss".
#include <math.h>

#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {
namespace {

constexpr int kVocThreads = 256;
constexpr int kVocWaves = kVocThreads / kWave;
constexpr int kFwdGroups = 2;                               // groups of four columns per thread of the forward
constexpr int kFwdCols = kVocThreads * 4 * kFwdGroups;      // 2048 columns per forward workgroup
constexpr int kBwdCols = kVocThreads * 4;                   // 1024 columns per backward workgroup
constexpr int kBwdRows = 8;                                 // rows per backward workgroup = rows of one grad_bias partial

// s[r, col0 .. col0 + 3]: one 16-byte load where the row allows it and the four columns exist, else dword loads; columns
// past the vocabulary read as -inf
template <int VEC>
__device__ __forceinline__ void load_scores(const float *__restrict__ row, const float *__restrict__ bias, int col0,
                                            int vocab, float (&v)[4]) {
  if (VEC == 4 && col0 + 4 <= vocab) {
    vec_load<4>(row + col0, v);
    if (bias) {
      float b[4];
      vec_load<4>(bias + col0, b);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += b[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = col0 + j;
      v[j] = c < vocab ? row[c] + (bias ? bias[c] : 0.0f) : -INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// a. forward
// ------------------------------------------------------------------------------------------------------------------
// Workgroup b: row b / chunks, columns kFwdCols (b % chunks) ..; partial[b] = (max, sum) of the chunk, target_score[r] =
// s[r, targets[r]] from the one thread that meets that column (a target outside [0, vocab) meets none).
template <int VEC>
__global__ __launch_bounds__(kVocThreads) void k_vocab_loss_partial(
    const float *__restrict__ scores, int64_t ld, int vocab, int chunks, const float *__restrict__ bias,
    const int64_t *__restrict__ targets, float2 *__restrict__ partial, float *__restrict__ target_score) {
  __shared__ MaxSum s_wave[kVocWaves];
  const int64_t r = blockIdx.x / chunks;
  const int c = (int)(blockIdx.x % chunks);
  const int t = threadIdx.x;
  const float *row = scores + r * ld;
  const int64_t tgt = targets ? targets[r] : -1;
  float v[kFwdGroups][4];
#pragma unroll
  for (int u = 0; u < kFwdGroups; ++u)
    load_scores<VEC>(row, bias, c * kFwdCols + u * (kVocThreads * 4) + 4 * t, vocab, v[u]);
  MaxSum a{-INFINITY, 0.0f};
#pragma unroll
  for (int u = 0; u < kFwdGroups; ++u) {
    const int col0 = c * kFwdCols + u * (kVocThreads * 4) + 4 * t;
    push4(a, v[u]);
    if (tgt >= col0 && tgt < col0 + 4 && tgt < vocab) target_score[r] = v[u][(int)(tgt - col0)];
  }
  a = waves_in_order<kVocWaves>(wave_fold(a, combine), s_wave, combine, t == 0);
  if (t == 0) partial[blockIdx.x] = make_float2(a.m, a.s);
}

// Thread per row: the chunks in chunk order, then the copy term and the picked entry.
__global__ __launch_bounds__(kVocThreads) void k_vocab_loss_merge(
    const float2 *__restrict__ partial, const float *__restrict__ target_score, int64_t rows, int vocab, int chunks,
    const float *__restrict__ extra, const int64_t *__restrict__ targets, float *__restrict__ norm,
    float *__restrict__ picked, float2 *__restrict__ stats) {
  const int64_t r = (int64_t)blockIdx.x * kVocThreads + threadIdx.x;
  if (r >= rows) return;
  const float2 *p = partial + r * chunks;
  MaxSum a{p[0].x, p[0].y};
  for (int c = 1; c < chunks; ++c) a = combine(a, MaxSum{p[c].x, p[c].y});
  if (extra) a = combine(a, MaxSum{extra[r], 1.0f});                   // extra = -inf: (max, sum) unchanged, bit for bit
  const float log_sum = a.m == -INFINITY ? 0.0f : logf(a.s);
  norm[r] = a.m + log_sum;
  stats[r] = make_float2(a.m, log_sum);
  if (targets && picked) {
    const int64_t tgt = targets[r];
    picked[r] = tgt >= 0 && tgt < vocab ? (target_score[r] - a.m) - log_sum : NAN;   // never an index: a visible nan
  }
}

// ------------------------------------------------------------------------------------------------------------------
// b. backward
// ------------------------------------------------------------------------------------------------------------------
// Workgroup b: row block b / chunks (kBwdRows rows), columns kBwdCols (b % chunks) .., thread t the columns 4 t .. 4 t + 3
// of the chunk.  part[row block, :] = the column sums of the block's rows, added in row order.
template <int VEC>
__global__ __launch_bounds__(kVocThreads) void k_vocab_loss_backward(
    const float *__restrict__ scores, int64_t ld, int64_t rows, int vocab, int chunks, const float *__restrict__ bias,
    const float *__restrict__ extra, const int64_t *__restrict__ targets, const float2 *__restrict__ stats,
    const float *__restrict__ g_norm, const float *__restrict__ g_picked, float *__restrict__ grad, int64_t ld_g,
    float *__restrict__ grad_extra, float *__restrict__ part, int64_t ld_part) {
  const int64_t rb = blockIdx.x / chunks;
  const int c = (int)(blockIdx.x % chunks);
  const int t = threadIdx.x;
  const int64_t row0 = rb * kBwdRows;
  const int col0 = c * kBwdCols + 4 * t;
  if (c == 0 && grad_extra && t < kBwdRows && row0 + t < rows) {
    const int64_t r = row0 + t;
    const float a = (g_norm ? g_norm[r] : 0.0f) - (g_picked ? g_picked[r] : 0.0f);
    const float2 st = stats[r];
    const float e = extra ? expf((extra[r] - st.x) - st.y) : 0.0f;
    grad_extra[r] = e == 0.0f ? 0.0f : a * e;
  }
  if (col0 >= vocab) return;
  const bool whole = VEC == 4 && col0 + 4 <= vocab;
  float v[kBwdRows][4];
#pragma unroll
  for (int i = 0; i < kBwdRows; ++i) {                      // rows past the end re-read the last row; nothing of them is kept
    const int64_t r = row0 + i < rows ? row0 + i : rows - 1;
    load_scores<VEC>(scores + r * ld, bias, col0, vocab, v[i]);
  }
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < kBwdRows; ++i) {
    const int64_t r = row0 + i;
    if (r >= rows) break;
    const float gp = g_picked ? g_picked[r] : 0.0f;
    const float a = (g_norm ? g_norm[r] : 0.0f) - gp;
    const float2 st = stats[r];
    const int64_t tgt = targets ? targets[r] : -1;
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      g[j] = a * expf((v[i][j] - st.x) - st.y) + (tgt == col0 + j ? gp : 0.0f);
      acc[j] += g[j];
    }
    float *out = grad + r * ld_g + col0;
    if (whole) {
      vec_store<4>(out, g);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col0 + j < vocab) out[j] = g[j];
    }
  }
  if (part) vec_store<4>(part + rb * ld_part + col0, acc);   // ld_part = vocab rounded up to 4: inside the partial's row
}

// grad_bias[v] = the row blocks' partials added in row-block order
__global__ __launch_bounds__(kVocThreads) void k_vocab_bias_fold(const float *__restrict__ part, int64_t ld_part,
                                                                  int row_blocks, int vocab,
                                                                  float *__restrict__ grad_bias) {
  const int j = blockIdx.x * kVocThreads + threadIdx.x;
  if (j >= vocab) return;
  grad_bias[j] = chunk_fold(part + j, ld_part, 0, row_blocks);
}

// ------------------------------------------------------------------------------------------------------------------
// c. the [B, L] tail (grucopydecoder.py:171-212)
// ------------------------------------------------------------------------------------------------------------------
// any = logsumexp(stack(gen', copied)) as torch computes it: the maximum (0 where it is infinite) taken out, no fused
// multiply-add (not log_add_exp of decode_common.h, which is log1p-based and guards only lo = -inf)
__device__ __forceinline__ float log_sum_exp2(float a, float b) {
  float m = fmaxf(a, b);
  if (fabsf(m) == INFINITY) m = 0.0f;
  return __fadd_rn(logf(__fadd_rn(expf(a - m), expf(b - m))), m);
}

__global__ __launch_bounds__(kVocThreads) void k_copy_loss_finish(
    const float *__restrict__ gen, const float *__restrict__ copied, const int32_t *__restrict__ rowptr,
    const int64_t *__restrict__ targets, int64_t unk_id, const int64_t *__restrict__ lengths, int num_samples,
    int steps, float *__restrict__ loss, float *__restrict__ d_gen, float *__restrict__ d_copied,
    float *__restrict__ per_sample) {
  __shared__ float s_run[kVocThreads];
  const int t = threadIdx.x;
  const float batch = (float)num_samples;
  for (int b = t; b < num_samples; b += kVocThreads) {
    const int64_t len = lengths[b];
    float total = 0.0f, count = 0.0f;
    for (int l = 0; l < steps; ++l) count += (int64_t)l < len ? 1.0f : 0.0f;
    for (int l = 0; l < steps; ++l) {                        // step order
      const int64_t r = (int64_t)b * steps + l;
      const bool has_copy = rowptr && rowptr[r + 1] > rowptr[r];
      const float g = has_copy && targets[r] == unk_id ? -INFINITY : gen[r];
      const float cp = copied[r];
      const float any = log_sum_exp2(g, cp);
      const float mask = (int64_t)l < len ? 1.0f : 0.0f;
      total = __fadd_rn(total, __fmul_rn(any, mask));
      // d loss / d any = -mask / (B count); softmax weights of the two terms, 0 where a term is -inf
      const float up = mask == 0.0f || any == -INFINITY ? 0.0f : -1.0f / (batch * count);
      d_gen[r] = up == 0.0f || g == -INFINITY ? 0.0f : up * expf(g - any);
      d_copied[r] = up == 0.0f || cp == -INFINITY ? 0.0f : up * expf(cp - any);
    }
    per_sample[b] = __fdiv_rn(total, count);
  }
  __syncthreads();
  const int per = (num_samples + kVocThreads - 1) / kVocThreads;
  const int lo = min(t * per, num_samples), hi = min(lo + per, num_samples);
  float run = 0.0f;
  for (int b = lo; b < hi; ++b) run += per_sample[b];        // sample order inside a run
  s_run[t] = run;
  __syncthreads();
  if (t != 0) return;
  float sum = 0.0f;
  for (int i = 0; i < kVocThreads; ++i) sum += s_run[i];     // runs in thread order
  loss[0] = -(sum / batch);
}

int64_t fwd_chunks(int32_t vocab) { return ((int64_t)vocab + kFwdCols - 1) / kFwdCols; }
int64_t bwd_chunks(int32_t vocab) { return ((int64_t)vocab + kBwdCols - 1) / kBwdCols; }
int64_t row_blocks(int64_t rows) { return (rows + kBwdRows - 1) / kBwdRows; }
int64_t part_ld(int32_t vocab) { return ((int64_t)vocab + 3) / 4 * 4; }

struct FwdWs {
  size_t partial, target_score, bytes;
};

FwdWs fwd_workspace(int64_t rows, int32_t vocab) {
  Carve c;
  FwdWs w;
  w.partial = c.take((size_t)rows * fwd_chunks(vocab) * sizeof(float2));
  w.target_score = c.take((size_t)rows * sizeof(float));
  w.bytes = c.off;
  return w;
}

size_t bwd_workspace(int64_t rows, int32_t vocab) {
  Carve c;
  c.take((size_t)row_blocks(rows) * part_ld(vocab) * sizeof(float));
  return c.off;
}

// what the two vocabulary entries share: sizes, and everything a kernel indexes with an int fits one
int vocab_check(const char *what, int64_t rows, int32_t vocab, int64_t ld) {
  PTGNN_REQUIRE(rows >= 0 && vocab >= 1, PTGNN_AMD_EINVAL, "%s: bad sizes (rows %lld, vocab %d)", what, (long long)rows,
                vocab);
  PTGNN_REQUIRE(ld >= vocab, PTGNN_AMD_EINVAL, "%s: leading dimension %lld < vocab %d", what, (long long)ld, vocab);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(vocab <= lim - 4 * kFwdCols && rows <= (lim - 1) / bwd_chunks(vocab), PTGNN_AMD_EUNSUPPORTED,
                "%s: too many rows / columns", what);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" size_t ptgnn_amd_vocab_loss_workspace_bytes(int64_t rows, int32_t vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  return fwd_workspace(rows, vocab).bytes;
}

extern "C" int ptgnn_amd_vocab_loss_f32(const float *scores, int64_t ld, int64_t rows, int32_t vocab, const float *bias,
                                        const float *extra, const int64_t *targets, float *norm, float *picked,
                                        float *stats, void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = vocab_check("vocab_loss", rows, vocab, ld)) return rc;
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(scores && norm && stats && (!targets || picked), PTGNN_AMD_EINVAL, "vocab_loss: null pointer");
  const FwdWs w = fwd_workspace(rows, vocab);
  if (const int rc = workspace_check("vocab_loss", workspace, workspace_bytes, w.bytes)) return rc;
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
                PTGNN_AMD_EINVAL, "vocab_loss: workspace and stats must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  const int chunks = (int)fwd_chunks(vocab);
  float2 *partial = carved<float2>(workspace, w.partial);
  float *target_score = carved<float>(workspace, w.target_score);
  const unsigned grid = (unsigned)(rows * chunks);
  if (ld % 4 == 0 && aligned16(scores) && aligned16(bias))
    k_vocab_loss_partial<4><<<grid, kVocThreads, 0, st>>>(scores, ld, vocab, chunks, bias, targets, partial, target_score);
  else
    k_vocab_loss_partial<1><<<grid, kVocThreads, 0, st>>>(scores, ld, vocab, chunks, bias, targets, partial, target_score);
  PTGNN_LAUNCH_CHECK();
  k_vocab_loss_merge<<<(unsigned)((rows + kVocThreads - 1) / kVocThreads), kVocThreads, 0, st>>>(
      partial, target_score, rows, vocab, chunks, extra, targets, norm, picked, reinterpret_cast<float2 *>(stats));
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_VOCAB_LOSS);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_vocab_loss_backward_workspace_bytes(int64_t rows, int32_t vocab) {
  if (rows <= 0 || vocab <= 0) return 0;
  return bwd_workspace(rows, vocab);
}

extern "C" int ptgnn_amd_vocab_loss_backward_f32(const float *scores, int64_t ld, int64_t rows, int32_t vocab,
                                                 const float *bias, const float *extra, const int64_t *targets,
                                                 const float *stats, const float *g_norm, const float *g_picked,
                                                 float *grad_scores, int64_t ld_g, float *grad_extra, float *grad_bias,
                                                 void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = vocab_check("vocab_loss_backward", rows, vocab, ld)) return rc;
  PTGNN_REQUIRE(ld_g >= vocab, PTGNN_AMD_EINVAL, "vocab_loss_backward: leading dimension %lld < vocab %d",
                (long long)ld_g, vocab);
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(scores && stats && grad_scores, PTGNN_AMD_EINVAL, "vocab_loss_backward: null pointer");
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, PTGNN_AMD_EINVAL,
                "vocab_loss_backward: stats must be 8-byte aligned");
  const float2 *row_stats = reinterpret_cast<const float2 *>(stats);
  if (grad_bias) {
    if (const int rc = workspace_check("vocab_loss_backward", workspace, workspace_bytes, bwd_workspace(rows, vocab)))
      return rc;
    PTGNN_REQUIRE(aligned16(workspace), PTGNN_AMD_EINVAL, "vocab_loss_backward: workspace must be 16-byte aligned");
  }
  hipStream_t st = (hipStream_t)stream_;
  const int chunks = (int)bwd_chunks(vocab);
  const int64_t blocks = row_blocks(rows);
  float *part = grad_bias ? static_cast<float *>(workspace) : nullptr;
  const unsigned grid = (unsigned)(blocks * chunks);
  if (ld % 4 == 0 && ld_g % 4 == 0 && aligned16(scores) && aligned16(bias) && aligned16(grad_scores))
    k_vocab_loss_backward<4><<<grid, kVocThreads, 0, st>>>(scores, ld, rows, vocab, chunks, bias, extra, targets, row_stats,
                                                          g_norm, g_picked, grad_scores, ld_g, grad_extra, part,
                                                          part_ld(vocab));
  else
    k_vocab_loss_backward<1><<<grid, kVocThreads, 0, st>>>(scores, ld, rows, vocab, chunks, bias, extra, targets, row_stats,
                                                          g_norm, g_picked, grad_scores, ld_g, grad_extra, part,
                                                          part_ld(vocab));
  PTGNN_LAUNCH_CHECK();
  if (grad_bias) {
    k_vocab_bias_fold<<<(unsigned)((vocab + kVocThreads - 1) / kVocThreads), kVocThreads, 0, st>>>(
        part, part_ld(vocab), (int)blocks, vocab, grad_bias);
    PTGNN_LAUNCH_CHECK();
  }
  count_launch(PTGNN_AMD_KERNEL_VOCAB_LOSS_BACKWARD);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_copy_loss_finish_workspace_bytes(int64_t num_samples) {
  if (num_samples <= 0) return 0;
  return (size_t)num_samples * sizeof(float);
}

extern "C" int ptgnn_amd_copy_loss_finish_f32(const float *gen, const float *copied, const int32_t *rowptr,
                                              const int64_t *targets, int64_t unk_id, const int64_t *lengths,
                                              int64_t num_samples, int32_t steps, float *loss, float *d_gen,
                                              float *d_copied, void *workspace, size_t workspace_bytes, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && steps >= 0, PTGNN_AMD_EINVAL, "copy_loss_finish: bad sizes (samples %lld, steps %d)",
                (long long)num_samples, steps);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_samples < lim && num_samples * (int64_t)steps < lim, PTGNN_AMD_EUNSUPPORTED,
                "copy_loss_finish: too many locations");
  if (num_samples == 0 || steps == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(gen && copied && targets && lengths && loss && d_gen && d_copied, PTGNN_AMD_EINVAL,
                "copy_loss_finish: null pointer");
  if (const int rc = workspace_check("copy_loss_finish", workspace, workspace_bytes,
                                     ptgnn_amd_copy_loss_finish_workspace_bytes(num_samples)))
    return rc;
  k_copy_loss_finish<<<1, kVocThreads, 0, (hipStream_t)stream_>>>(gen, copied, rowptr, targets, unk_id, lengths,
                                                                   (int)num_samples, steps, loss, d_gen, d_copied,
                                                                   static_cast<float *>(workspace));
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_COPY_LOSS_FINISH);
  return PTGNN_AMD_OK;
}
