// The task heads of the three benchmarked models: what the reference runs AFTER its GNN to turn node states into a loss
// and an accuracy figure.
//
//   Graph2ClassModule    ptgnn/implementations/typilus/graph2class.py:81-102      nn.CrossEntropyLoss over [S, C] logits,
//                                                                                  argmax accuracy, softmax max for predict()
//   PPIClassification    ptgnn/implementations/ppi/ppi.py:37-62                    sigmoid >= 0.5, tp / fp / fn, precision,
//                                                                                  recall, F1, BCE-with-logits summed per row
//   VarMisuseGraphModel  ptgnn/implementations/varmisuse/varmisuse.py:58-91        gather candidates and slots, cat,
//                                                                                  Linear(2H, 1), scatter_log_softmax(eps=0),
//                                                                                  scatter_max accuracy, NLL of the correct one
//
// Two kernel families, exact fp32, no float atomics.
//
// a. ROW LOSS OVER A LOGIT MATRIX (logit_loss).  Rows are cut into the 128-row chunks of segment_chunks.h (one segment: all
//    rows); a workgroup takes a chunk, a wave a row.  Mode 0 (softmax cross-entropy) walks the row ONCE with a running
//    (max, sum, arg-max) per lane, merges the lanes (Soft of softmax_state.h) and reads logit[target] directly.
//    Mode 1 (sigmoid / BCE) adds max(l, 0) - l t + log1p(exp(-|l|)) and counts tp / fp / fn with the prediction l >= 0.
//    Every logit is read from HBM once per pass, whatever C.  A chunk leaves (loss sum as float64 | three int64 counts);
//    k_logit_merge adds the chunks IN CHUNK ORDER (thread t the t-th contiguous run of chunks, thread 0 the runs in thread
//    order), writes the totals block and the loss, and adds into the caller's persistent metrics block.
//    The backward is one more pass: grad = g / live (softmax - onehot), or g / R (sigmoid - t), with g and the
//    denominator read from DEVICE memory.
//
// b. CANDIDATE SCORING OVER A SEGMENT MAP (candidate_scores).  A workgroup per slot: every wave dots the slot's row with
//    w[D:], then the four waves walk the slot's candidates in plan order (wave v the candidates v, v + 4, ...), dot each
//    gathered row with w[:D], write the score and keep a running (max, sum, arg-max position); thread 0 merges the four
//    waves in wave order.  A slot's lse and arg-max are a fixed function of ITS candidates and their plan order.  The
//    merge launch forms score[correct_g] - lse[g] per slot and folds the slots in slot order.  The backward walks the
//    candidates of a slot serially in plan order with a thread per column: t_c, the candidate row t_c w[:D], the slot
//    row (sum t_c) w[D:] and the slot's two halves of dw; the slots' halves are then added in slot order.
//
// Traffic: DESIGN.md, "Task heads".
#include <limits.h>
#include <math.h>

#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {
namespace {

constexpr int kHeadThreads = 256;
constexpr int kHeadWaves = kHeadThreads / kWave;
constexpr int kPartSlots = 4;          // a chunk's partial: loss sum (float64 bits) | three int64 counts
constexpr int kCandMaxDim = 1024;

// totals block, 8-byte slots (PTGNN_AMD_HEAD_TOTALS_BYTES = 64): see include/ptgnn_amd.h
enum { kTotSum = 0, kTotDenom = 1, kTotA = 2, kTotB = 3, kTotC = 4, kTotRows = 5 };

// ------------------------------------------------------------------------------------------------------------------
// a. logit loss
// ------------------------------------------------------------------------------------------------------------------
// Workgroup b: rows 128 b .. 128 b + 127, wave v the rows v, v + 4, ...  partial[b, 0:4] = loss sum | c0 | c1 | c2 with
//   mode 0: c0 live rows, c1 rows whose arg-max is their target, c2 rows with a target outside [0, C) other than -100
//   mode 1: c0 true positives, c1 false positives, c2 false negatives
template <int MODE>
__global__ __launch_bounds__(kHeadThreads) void k_logit_loss(
    const float *__restrict__ logits, int64_t ld, int64_t rows, int classes, const int64_t *__restrict__ target_ids,
    const uint8_t *__restrict__ target_bits, int64_t ld_t, float *__restrict__ lse, int64_t *__restrict__ argmax,
    float *__restrict__ max_prob, float *__restrict__ row_loss, int64_t *__restrict__ partial) {
  __shared__ float s_loss[kChunkRows];
  __shared__ int s_c[3][kChunkRows];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kChunkRows;
  for (int i = wave; i < kChunkRows; i += kHeadWaves) {
    const int64_t r = row0 + i;
    float loss = 0.0f;
    int c0 = 0, c1 = 0, c2 = 0;
    if (r < rows) {
      const float *row = logits + r * ld;
      if constexpr (MODE == 0) {
        Soft a = soft_empty();
        for (int c = lane; c < classes; c += kWave) soft_push(a, row[c], c);
        a = wave_fold(a, soft_merge);
        const float l = a.m + logf(a.s);
        if (lane == 0) {
          lse[r] = l;
          if (argmax) argmax[r] = a.idx;
          if (max_prob) max_prob[r] = expf(a.m - l);
        }
        if (target_ids) {
          const int64_t tgt = target_ids[r];
          const bool live = tgt >= 0 && tgt < classes;
          if (live) loss = l - row[tgt];
          c0 = live ? 1 : 0;
          c1 = live && tgt == a.idx ? 1 : 0;
          c2 = !live && tgt != -100 ? 1 : 0;
        }
      } else {
        const uint8_t *tr = target_bits + r * ld_t;
        float part = 0.0f;
        int tp = 0, fp = 0, fn = 0;
        for (int c = lane; c < classes; c += kWave) {
          const float l = row[c];
          const bool t = tr[c] != 0, p = l >= 0.0f;
          part += (fmaxf(l, 0.0f) - (t ? l : 0.0f)) + log1pf(expf(-fabsf(l)));
          tp += p && t ? 1 : 0;
          fp += p && !t ? 1 : 0;
          fn += !p && t ? 1 : 0;
        }
        loss = group_sum(part);
        c0 = group_sum(tp);
        c1 = group_sum(fp);
        c2 = group_sum(fn);
      }
      if (lane == 0 && row_loss) row_loss[r] = loss;
    }
    if (lane == 0) {
      s_loss[i] = loss;
      s_c[0][i] = c0;
      s_c[1][i] = c1;
      s_c[2][i] = c2;
    }
  }
  __syncthreads();
  if (wave == 0) {                     // the chunk's rows in a fixed tree: lane l adds rows l and l + 64, then the butterfly
    const double l = group_sum((double)s_loss[lane] + (double)s_loss[lane + kWave]);
    const int a = group_sum(s_c[0][lane] + s_c[0][lane + kWave]);
    const int b = group_sum(s_c[1][lane] + s_c[1][lane + kWave]);
    const int c = group_sum(s_c[2][lane] + s_c[2][lane + kWave]);
    if (lane == 0) {
      int64_t *out = partial + (int64_t)blockIdx.x * kPartSlots;
      out[0] = __double_as_longlong(l);
      out[1] = a;
      out[2] = b;
      out[3] = c;
    }
  }
}

// The chunks of [0, n) added in chunk order by ONE workgroup: thread t adds the t-th contiguous run, thread k < 4 then adds
// the 256 runs of slot k in thread order.  sum[0] is the float64 loss sum, sum[1..3] the counts.
struct MergeLds {
  double d[kHeadThreads];
  int64_t c[3][kHeadThreads];
  double sum_d;
  int64_t sum_c[3];
};

__device__ __forceinline__ void merge_runs(MergeLds &m, double d, int64_t a, int64_t b, int64_t c) {
  const int t = threadIdx.x;
  m.d[t] = d;
  m.c[0][t] = a;
  m.c[1][t] = b;
  m.c[2][t] = c;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < kHeadThreads; ++i) s += m.d[i];
    m.sum_d = s;
  } else if (t <= 3) {
    int64_t s = 0;
    for (int i = 0; i < kHeadThreads; ++i) s += m.c[t - 1][i];
    m.sum_c[t - 1] = s;
  }
  __syncthreads();
}

// precision / recall / F-score of ppi.py:46-52, in the reference's fp32 arithmetic (no contraction)
__device__ __forceinline__ void prf(int64_t tp_, int64_t fp_, int64_t fn_, float &pr, float &re, float &f1) {
  const float tp = (float)tp_, fp = (float)fp_, fn = (float)fn_;
  pr = __fdiv_rn(tp, __fadd_rn(__fadd_rn(tp, fp), 1e-10f));
  re = __fdiv_rn(tp, __fadd_rn(__fadd_rn(tp, fn), 1e-10f));
  f1 = __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, pr), re), __fadd_rn(__fadd_rn(pr, re), 1e-10f));
}

__global__ __launch_bounds__(kHeadThreads) void k_logit_merge(const int64_t *__restrict__ partial, int chunks,
                                                              int64_t rows, int mode, float *__restrict__ loss,
                                                              int64_t *__restrict__ totals,
                                                              int64_t *__restrict__ metrics) {
  __shared__ MergeLds m;
  const int per = (chunks + kHeadThreads - 1) / kHeadThreads;
  const int lo = min((int)threadIdx.x * per, chunks), hi = min(lo + per, chunks);
  double d = 0.0;
  int64_t a = 0, b = 0, c = 0;
  for (int ch = lo; ch < hi; ++ch) {
    const int64_t *p = partial + (int64_t)ch * kPartSlots;
    d += __longlong_as_double(p[0]);
    a += p[1];
    b += p[2];
    c += p[3];
  }
  merge_runs(m, d, a, b, c);
  if (threadIdx.x != 0) return;
  d = m.sum_d;
  a = m.sum_c[0];
  b = m.sum_c[1];
  c = m.sum_c[2];
  const int64_t denom = mode == 0 ? a : rows;
  totals[kTotSum] = __double_as_longlong(d);
  totals[kTotDenom] = denom;
  totals[kTotA] = mode == 0 ? b : a;               // mode 0: correct | bad targets | 0;  mode 1: tp | fp | fn
  totals[kTotB] = mode == 0 ? c : b;
  totals[kTotC] = mode == 0 ? 0 : c;
  totals[kTotRows] = rows;
  totals[6] = totals[7] = 0;
  *loss = (float)(d / (double)denom);              // nan when every row is ignored, as nn.CrossEntropyLoss
  if (!metrics) return;
  if (mode == 0) {
    metrics[0] += b;
    metrics[1] += a;
    metrics[2] += c;
  } else {
    float pr, re, f1;
    prf(a, b, c, pr, re, f1);
    const double n = (double)rows;
    metrics[0] = __double_as_longlong(__longlong_as_double(metrics[0]) + (double)pr * n);
    metrics[1] = __double_as_longlong(__longlong_as_double(metrics[1]) + (double)re * n);
    metrics[2] = __double_as_longlong(__longlong_as_double(metrics[2]) + (double)f1 * n);
    metrics[3] += rows;
  }
}

template <int MODE>
__global__ __launch_bounds__(kHeadThreads) void k_logit_loss_backward(
    const float *__restrict__ logits, int64_t ld, int64_t rows, int classes, const int64_t *__restrict__ target_ids,
    const uint8_t *__restrict__ target_bits, int64_t ld_t, const float *__restrict__ lse,
    const int64_t *__restrict__ totals, const float *__restrict__ grad_loss, float *__restrict__ grad, int64_t ld_g) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kChunkRows;
  const float scale = grad_loss[0] / (float)totals[kTotDenom];
  for (int i = wave; i < kChunkRows; i += kHeadWaves) {
    const int64_t r = row0 + i;
    if (r >= rows) break;
    const float *row = logits + r * ld;
    float *out = grad + r * ld_g;
    if constexpr (MODE == 0) {
      const int64_t tgt = target_ids[r];
      const bool live = tgt >= 0 && tgt < classes;
      const float l = lse[r];
      for (int c = lane; c < classes; c += kWave)
        out[c] = live ? scale * (expf(row[c] - l) - (c == tgt ? 1.0f : 0.0f)) : 0.0f;
    } else {
      const uint8_t *tr = target_bits + r * ld_t;
      for (int c = lane; c < classes; c += kWave) {
        const float v = row[c];
        const float e = expf(-fabsf(v));                    // sigmoid without overflow
        const float sig = v >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        out[c] = scale * (sig - (tr[c] != 0 ? 1.0f : 0.0f));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// b. candidate scores
// ------------------------------------------------------------------------------------------------------------------
// a . b over `dim` columns by one wave: lane l takes the units l, l + 64, ... in order, then the butterfly
template <int VEC>
__device__ __forceinline__ float wave_dot(const float *__restrict__ a, const float *__restrict__ b, int dim, int lane) {
  float acc = 0.0f;
  for (int u = lane * VEC; u < dim; u += kWave * VEC) {
    float av[VEC], bv[VEC];
    vec_load<VEC>(a + u, av);
    vec_load<VEC>(b + u, bv);
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc = fmaf(av[v], bv[v], acc);
  }
  return group_sum(acc);
}

// row id clamped into [0, num_nodes); `bad` counts the ids that were outside
__device__ __forceinline__ int64_t clamp_node(int64_t id, int64_t num_nodes, int &bad) {
  if (id < 0 || id >= num_nodes) {
    ++bad;
    return id < 0 ? 0 : num_nodes - 1;
  }
  return id;
}

template <int VEC>
__global__ __launch_bounds__(kHeadThreads) void k_candidate_scores(
    const float *__restrict__ x, int64_t ld_x, int64_t num_nodes, const int64_t *__restrict__ cand_idx,
    const int64_t *__restrict__ slot_idx, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ perm,
    const float *__restrict__ w, int dim, int num_candidates, float *__restrict__ scores, float *__restrict__ lse,
    int64_t *__restrict__ argmax, int32_t *__restrict__ bad_part) {
  __shared__ Soft s_run[kHeadWaves];
  __shared__ int s_bad[kHeadWaves];
  const int g = blockIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int bad = 0, bad_slot = 0;
  const int64_t sn = clamp_node(slot_idx[g], num_nodes, bad_slot);
  const float sd = wave_dot<VEC>(x + sn * ld_x, w + dim, dim, lane);
  const int lo = max(rowptr[g], 0), hi = min(rowptr[g + 1], num_candidates);
  Soft run = soft_empty();
  for (int p = lo + wave; p < hi; p += kHeadWaves) {
    const int c = perm[p];
    if ((unsigned)c >= (unsigned)num_candidates) continue;      // never index with a slot the plan should not hold
    const int64_t nd = clamp_node(cand_idx[c], num_nodes, bad);
    const float sc = __fadd_rn(wave_dot<VEC>(x + nd * ld_x, w, dim, lane), sd);
    if (lane == 0) scores[c] = sc;
    soft_push_lowest(run, sc, c);                                // plan order: not ascending in c
  }
  if (lane == 0) s_bad[wave] = bad;
  const Soft a = waves_in_order<kHeadWaves>(run, s_run, soft_merge, threadIdx.x == 0);
  if (threadIdx.x == 0) {
    int nb = s_bad[0] + bad_slot;
    for (int v = 1; v < kHeadWaves; ++v) nb += s_bad[v];
    lse[g] = a.idx == kSoftNone ? -INFINITY : a.m + logf(a.s);
    argmax[g] = a.idx == kSoftNone ? (int64_t)num_candidates : (int64_t)a.idx;
    bad_part[g] = nb;
  }
}

// Per slot g with k = correct[g]: the term score[k] - lse[g] when k is a candidate OF SLOT g, a hit when it is the slot's
// arg-max; any other k is counted and skipped.  Slots folded in slot order (merge_runs).
__global__ __launch_bounds__(kHeadThreads) void k_candidate_merge(
    const float *__restrict__ scores, const float *__restrict__ lse, const int64_t *__restrict__ argmax,
    const int64_t *__restrict__ cand_slot, const int64_t *__restrict__ correct, const int32_t *__restrict__ bad_part,
    int num_candidates, int num_slots, float *__restrict__ loss, int64_t *__restrict__ totals,
    int64_t *__restrict__ metrics) {
  __shared__ MergeLds m;
  const int per = (num_slots + kHeadThreads - 1) / kHeadThreads;
  const int lo = min((int)threadIdx.x * per, num_slots), hi = min(lo + per, num_slots);
  double d = 0.0;
  int64_t hits = 0, bad_correct = 0, bad_nodes = 0;
  for (int g = lo; g < hi; ++g) {
    bad_nodes += bad_part[g];
    if (!correct) continue;
    const int64_t k = correct[g];
    const bool ok = k >= 0 && k < num_candidates && cand_slot[k] == g;
    if (ok) {
      d += (double)(scores[k] - lse[g]);
      hits += argmax[g] == k ? 1 : 0;
    } else {
      ++bad_correct;
    }
  }
  merge_runs(m, d, hits, bad_correct, bad_nodes);
  if (threadIdx.x != 0) return;
  totals[kTotSum] = __double_as_longlong(m.sum_d);
  totals[kTotDenom] = num_slots;
  totals[kTotA] = m.sum_c[0];
  totals[kTotB] = m.sum_c[1];
  totals[kTotC] = m.sum_c[2];
  totals[kTotRows] = num_candidates;
  totals[6] = totals[7] = 0;
  if (!correct) return;
  *loss = (float)(-m.sum_d / (double)num_slots);
  if (metrics) {
    metrics[0] += m.sum_c[0];
    metrics[1] += num_slots;
    metrics[2] += m.sum_c[1];
  }
}

// Workgroup g, thread t the columns t, t + 256, ...; the slot's candidates serially in plan order.
//   row_grad[c, :]        = t_c w[:D]                  dw_part[g, :D] = sum_c t_c x[cand_c, :]
//   row_grad[Cn + g, :]   = (sum_c t_c) w[D:]          dw_part[g, D:] = (sum_c t_c) x[slot_g, :]
template <int COLS>
__global__ __launch_bounds__(kHeadThreads) void k_candidate_scores_backward(
    const float *__restrict__ x, int64_t ld_x, int64_t num_nodes, const int64_t *__restrict__ cand_idx,
    const int64_t *__restrict__ slot_idx, const int64_t *__restrict__ cand_slot, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ perm, const float *__restrict__ w, const int64_t *__restrict__ correct,
    const float *__restrict__ scores, const float *__restrict__ lse, const float *__restrict__ grad_loss,
    const float *__restrict__ grad_scores, int dim, int num_candidates, int num_slots, float *__restrict__ row_grad,
    float *__restrict__ dw_part) {
  const int g = blockIdx.x, t = threadIdx.x;
  int unused = 0;
  const int64_t k = correct ? correct[g] : -1;
  const bool ok = k >= 0 && k < num_candidates && cand_slot[k] == g;
  const float scale = grad_loss ? grad_loss[0] / (float)num_slots : 0.0f;
  const float l = lse[g];
  float wc[COLS], wsl[COLS], acc[COLS];
#pragma unroll
  for (int q = 0; q < COLS; ++q) {
    const int col = t + q * kHeadThreads;
    wc[q] = col < dim ? w[col] : 0.0f;
    wsl[q] = col < dim ? w[dim + col] : 0.0f;
    acc[q] = 0.0f;
  }
  float tsum = 0.0f;
  const int lo = max(rowptr[g], 0), hi = min(rowptr[g + 1], num_candidates);
  for (int p = lo; p < hi; ++p) {
    const int c = perm[p];
    if ((unsigned)c >= (unsigned)num_candidates) continue;
    const int64_t nd = clamp_node(cand_idx[c], num_nodes, unused);
    // a slot whose correct index was skipped (or a call without `correct`) held no term of the loss: no loss gradient
    const float soft = ok && scale != 0.0f ? scale * (expf(scores[c] - l) - (c == k ? 1.0f : 0.0f)) : 0.0f;
    const float tc = soft + (grad_scores ? grad_scores[c] : 0.0f);
    tsum += tc;
    const float *xr = x + nd * ld_x;
    float *out = row_grad + (int64_t)c * dim;
#pragma unroll
    for (int q = 0; q < COLS; ++q) {
      const int col = t + q * kHeadThreads;
      if (col < dim) {
        acc[q] = fmaf(tc, xr[col], acc[q]);
        out[col] = tc * wc[q];
      }
    }
  }
  const int64_t sn = clamp_node(slot_idx[g], num_nodes, unused);
  const float *xs = x + sn * ld_x;
  float *out = row_grad + ((int64_t)num_candidates + g) * dim;
  float *part = dw_part + (int64_t)g * 2 * dim;
#pragma unroll
  for (int q = 0; q < COLS; ++q) {
    const int col = t + q * kHeadThreads;
    if (col < dim) {
      out[col] = tsum * wsl[q];
      part[col] = acc[q];
      part[dim + col] = tsum * xs[col];
    }
  }
}

// dw[j] = the slots' partials added in slot order
__global__ __launch_bounds__(256) void k_candidate_fold_dw(const float *__restrict__ dw_part, int num_slots, int width,
                                                            float *__restrict__ dw) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= width) return;
  dw[j] = chunk_fold(dw_part + j, (int64_t)width, 0, num_slots);
}

bool candidate_supported(int dim) { return dim >= 4 && dim <= kCandMaxDim && dim % 4 == 0; }

int64_t logit_chunks(int64_t rows) { return (rows + kChunkRows - 1) / kChunkRows; }

int logit_check(const char *what, int64_t rows, int32_t classes, int mode) {
  PTGNN_REQUIRE(rows >= 0 && classes >= 1 && (mode == 0 || mode == 1), PTGNN_AMD_EINVAL, "%s: bad sizes or mode", what);
  PTGNN_REQUIRE(logit_chunks(rows) < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many rows", what);
  return PTGNN_AMD_OK;
}

int candidate_check(const char *what, int64_t num_nodes, int64_t num_candidates, int64_t num_slots, int32_t dim) {
  PTGNN_REQUIRE(num_nodes >= 0 && num_candidates >= 0 && num_slots >= 0 && dim > 0, PTGNN_AMD_EINVAL, "%s: bad sizes",
                what);
  PTGNN_REQUIRE(candidate_supported(dim), PTGNN_AMD_EUNSUPPORTED,
                "%s: dim %d outside the kernel range (a multiple of 4, 4 <= dim <= %d)", what, dim, kCandMaxDim);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_candidates < lim && num_slots < lim / (2 * (int64_t)dim), PTGNN_AMD_EUNSUPPORTED,
                "%s: too many candidates / slots", what);
  PTGNN_REQUIRE(num_slots == 0 || num_nodes > 0, PTGNN_AMD_EINVAL, "%s: slots without nodes", what);
  return PTGNN_AMD_OK;
}

size_t candidate_backward_workspace(int64_t num_slots, int32_t dim) {
  Carve c;
  c.take((size_t)num_slots * 2 * dim * sizeof(float));
  return c.off;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" size_t ptgnn_amd_logit_loss_workspace_bytes(int64_t rows) {
  if (rows <= 0) return 0;
  return (size_t)logit_chunks(rows) * kPartSlots * sizeof(int64_t);
}

extern "C" int ptgnn_amd_logit_loss_f32(const float *logits, int64_t ld, int64_t rows, int32_t classes, int mode,
                                        const void *targets, int64_t ld_t, float *lse, int64_t *argmax,
                                        float *max_prob, float *row_loss, float *loss, void *totals, void *metrics,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = logit_check("logit_loss", rows, classes, mode)) return rc;
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(logits && ld >= classes, PTGNN_AMD_EINVAL, "logit_loss: null pointer or bad leading dimension");
  PTGNN_REQUIRE(mode == 1 || lse, PTGNN_AMD_EINVAL, "logit_loss: mode 0 needs lse");
  PTGNN_REQUIRE(mode == 0 || (targets && ld_t >= classes), PTGNN_AMD_EINVAL,
                "logit_loss: mode 1 needs targets with a leading dimension >= classes");
  PTGNN_REQUIRE(!targets || (loss && totals), PTGNN_AMD_EINVAL, "logit_loss: targets need loss and totals");
  const int64_t chunks = logit_chunks(rows);
  if (const int rc = workspace_check("logit_loss", workspace, workspace_bytes,
                                     ptgnn_amd_logit_loss_workspace_bytes(rows)))
    return rc;
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(totals) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(metrics) & 7u) == 0,
                PTGNN_AMD_EINVAL, "logit_loss: workspace, totals and metrics must be 8-byte aligned");
  int64_t *partial = static_cast<int64_t *>(workspace);   // predict (no targets): the partials are written, not merged
  hipStream_t st = (hipStream_t)stream_;
  if (mode == 0)
    k_logit_loss<0><<<(unsigned)chunks, kHeadThreads, 0, st>>>(logits, ld, rows, classes,
                                                                static_cast<const int64_t *>(targets), nullptr, 0, lse,
                                                                argmax, max_prob, row_loss, partial);
  else
    k_logit_loss<1><<<(unsigned)chunks, kHeadThreads, 0, st>>>(logits, ld, rows, classes, nullptr,
                                                                static_cast<const uint8_t *>(targets), ld_t, nullptr,
                                                                nullptr, nullptr, row_loss, partial);
  PTGNN_LAUNCH_CHECK();
  if (targets) {
    k_logit_merge<<<1, kHeadThreads, 0, st>>>(partial, (int)chunks, rows, mode, loss, static_cast<int64_t *>(totals),
                                              static_cast<int64_t *>(metrics));
    PTGNN_LAUNCH_CHECK();
  }
  count_launch(PTGNN_AMD_KERNEL_LOGIT_LOSS);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_logit_loss_backward_f32(const float *logits, int64_t ld, int64_t rows, int32_t classes,
                                                 int mode, const void *targets, int64_t ld_t, const float *lse,
                                                 const void *totals, const float *grad_loss, float *grad_logits,
                                                 int64_t ld_g, void *stream_) {
  if (const int rc = logit_check("logit_loss_backward", rows, classes, mode)) return rc;
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(logits && targets && totals && grad_loss && grad_logits && (mode == 1 || lse), PTGNN_AMD_EINVAL,
                "logit_loss_backward: null pointer");
  PTGNN_REQUIRE(ld >= classes && ld_g >= classes && (mode == 0 || ld_t >= classes), PTGNN_AMD_EINVAL,
                "logit_loss_backward: bad leading dimension");
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(totals) & 7u) == 0, PTGNN_AMD_EINVAL,
                "logit_loss_backward: totals must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  const unsigned grid = (unsigned)logit_chunks(rows);
  if (mode == 0)
    k_logit_loss_backward<0><<<grid, kHeadThreads, 0, st>>>(logits, ld, rows, classes,
                                                            static_cast<const int64_t *>(targets), nullptr, 0, lse,
                                                            static_cast<const int64_t *>(totals), grad_loss, grad_logits,
                                                            ld_g);
  else
    k_logit_loss_backward<1><<<grid, kHeadThreads, 0, st>>>(logits, ld, rows, classes, nullptr,
                                                            static_cast<const uint8_t *>(targets), ld_t, nullptr,
                                                            static_cast<const int64_t *>(totals), grad_loss, grad_logits,
                                                            ld_g);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_LOGIT_LOSS_BACKWARD);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_candidate_scores_supported(int32_t dim) { return candidate_supported(dim) ? 1 : 0; }

extern "C" size_t ptgnn_amd_candidate_scores_workspace_bytes(int64_t num_slots) {
  if (num_slots <= 0) return 0;
  return (size_t)num_slots * sizeof(int32_t);
}

extern "C" int ptgnn_amd_candidate_scores_f32(const float *x, int64_t ld_x, int64_t num_nodes, const int64_t *cand_idx,
                                              const int64_t *slot_idx, const int64_t *cand_slot, const int32_t *rowptr,
                                              const int32_t *perm, int64_t num_candidates, int64_t num_slots,
                                              int32_t dim, const float *w, const int64_t *correct, float *scores,
                                              float *lse, int64_t *argmax, float *loss, void *totals, void *metrics,
                                              void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = candidate_check("candidate_scores", num_nodes, num_candidates, num_slots, dim)) return rc;
  if (num_slots == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && slot_idx && rowptr && w && lse && argmax && totals &&
                    (num_candidates == 0 || (cand_idx && cand_slot && perm && scores)),
                PTGNN_AMD_EINVAL, "candidate_scores: null pointer");
  PTGNN_REQUIRE(!correct || loss, PTGNN_AMD_EINVAL, "candidate_scores: correct needs loss");
  PTGNN_REQUIRE(ld_x >= dim, PTGNN_AMD_EINVAL, "candidate_scores: bad leading dimension");
  PTGNN_REQUIRE((reinterpret_cast<uintptr_t>(totals) & 7u) == 0 && (reinterpret_cast<uintptr_t>(metrics) & 7u) == 0,
                PTGNN_AMD_EINVAL, "candidate_scores: totals and metrics must be 8-byte aligned");
  if (const int rc = workspace_check("candidate_scores", workspace, workspace_bytes,
                                     ptgnn_amd_candidate_scores_workspace_bytes(num_slots)))
    return rc;
  hipStream_t st = (hipStream_t)stream_;
  int32_t *bad_part = static_cast<int32_t *>(workspace);
  const bool vec4 = ld_x % 4 == 0 && aligned16(x) && aligned16(w);
  if (vec4)
    k_candidate_scores<4><<<(unsigned)num_slots, kHeadThreads, 0, st>>>(x, ld_x, num_nodes, cand_idx, slot_idx, rowptr,
                                                                         perm, w, dim, (int)num_candidates, scores, lse,
                                                                         argmax, bad_part);
  else
    k_candidate_scores<1><<<(unsigned)num_slots, kHeadThreads, 0, st>>>(x, ld_x, num_nodes, cand_idx, slot_idx, rowptr,
                                                                         perm, w, dim, (int)num_candidates, scores, lse,
                                                                         argmax, bad_part);
  PTGNN_LAUNCH_CHECK();
  k_candidate_merge<<<1, kHeadThreads, 0, st>>>(scores, lse, argmax, cand_slot, correct, bad_part, (int)num_candidates,
                                                (int)num_slots, loss, static_cast<int64_t *>(totals),
                                                static_cast<int64_t *>(metrics));
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_CANDIDATE_SCORES);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_candidate_scores_backward_workspace_bytes(int64_t num_slots, int32_t dim) {
  if (num_slots <= 0 || dim <= 0) return 0;
  return candidate_backward_workspace(num_slots, dim);
}

#define CANDIDATE_BACKWARD(COLS_)                                                                                      \
  k_candidate_scores_backward<COLS_><<<(unsigned)num_slots, kHeadThreads, 0, st>>>(                                    \
      x, ld_x, num_nodes, cand_idx, slot_idx, cand_slot, rowptr, perm, w, correct, scores, lse, grad_loss, grad_scores, \
      dim, (int)num_candidates, (int)num_slots, row_grad, dw_part)

extern "C" int ptgnn_amd_candidate_scores_backward_f32(const float *x, int64_t ld_x, int64_t num_nodes,
                                                       const int64_t *cand_idx, const int64_t *slot_idx,
                                                       const int64_t *cand_slot, const int32_t *rowptr,
                                                       const int32_t *perm, int64_t num_candidates, int64_t num_slots,
                                                       int32_t dim, const float *w, const int64_t *correct,
                                                       const float *scores, const float *lse, const float *grad_loss,
                                                       const float *grad_scores, float *row_grad, float *grad_w,
                                                       void *workspace, size_t workspace_bytes, void *stream_) {
  if (const int rc = candidate_check("candidate_scores_backward", num_nodes, num_candidates, num_slots, dim)) return rc;
  PTGNN_REQUIRE(grad_w, PTGNN_AMD_EINVAL, "candidate_scores_backward: null pointer");
  hipStream_t st = (hipStream_t)stream_;
  if (num_slots == 0) {
    PTGNN_HIP(hipMemsetAsync(grad_w, 0, (size_t)2 * dim * sizeof(float), st));
    return PTGNN_AMD_OK;
  }
  PTGNN_REQUIRE(x && slot_idx && rowptr && w && lse && row_grad &&
                    (num_candidates == 0 || (cand_idx && cand_slot && perm && scores)),
                PTGNN_AMD_EINVAL, "candidate_scores_backward: null pointer");
  PTGNN_REQUIRE(ld_x >= dim, PTGNN_AMD_EINVAL, "candidate_scores_backward: bad leading dimension");
  if (const int rc = workspace_check("candidate_scores_backward", workspace, workspace_bytes,
                                     candidate_backward_workspace(num_slots, dim)))
    return rc;
  float *dw_part = static_cast<float *>(workspace);
  if (dim <= 256) CANDIDATE_BACKWARD(1);
  else if (dim <= 512) CANDIDATE_BACKWARD(2);
  else CANDIDATE_BACKWARD(4);
  PTGNN_LAUNCH_CHECK();
  k_candidate_fold_dw<<<(unsigned)((2 * dim + 255) / 256), 256, 0, st>>>(dw_part, (int)num_slots, 2 * dim, grad_w);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_CANDIDATE_SCORES_BACKWARD);
  return PTGNN_AMD_OK;
}
