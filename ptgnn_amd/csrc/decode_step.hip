// One step of the copying decoder's greedy decoding (ptgnn/neuralmodels/sequence/grucopydecoder.py:375-457) in ONE launch:
// from the RAW output of the second vocabulary Linear and the copy scores of the step straight to the predicted token,
// its log-probability and the next input token.  Neither `target_logprobs` [B, V] nor `copy_logprobs` [I] exists, nothing
// is ranked, nothing visits the host.  With s[b, v] = scores[b, v] + bias[v], c[i] the copy score of memory i,
// norm[b] = logaddexp(log sum_v exp s[b, v], total_copy[b]) and K = top_k, the reference's dict of sample b holds
//     the K largest s[b, .] - norm[b]                                              (torch.topk)
//     merged with, per VALUE id g among the sample's memories, log sum_{i in b, id(i) = g} exp(c[i] - norm[b]) by logaddexp
//     -- onto the vocabulary entry when g < V and that entry is one of the K, else onto -inf
// and predicts its arg-max.  Only two kinds of entry can win: the row's top-1 and the merged entries of the sample's
// value groups.  So a sample needs the normaliser, the top-1, and for each group with g < V whether s[b, g] is one of the
// K largest: a comparison with the K-th largest value of the row.
//
// One workgroup of kDecThreads threads per sample (B is about 50 and V at most about 20 000: the launch is bound by the
// latency of one row, not by the chip; a row split over workgroups would need a second launch or a cross-workgroup
// hand-off for 80 KB of L2-resident reads).  Thread t owns the columns t, t + kDecThreads, ... in every pass.
//   1. One pass over the row: the running (maximum, sum) of csrc/softmax_state.h, its threads and waves merged as that
//      header says, joined with the copy term, and the top-1 (value, lowest index).
//   2. K < V only: the K-th largest value by a radix select, eight bits a pass, over the order-preserving bit pattern of
//      the floats (-0 counted as +0), a 256-bin histogram in LDS counted with INTEGER atomics (their result does not
//      depend on the order of arrival); the row is re-read from L2.  Entries equal to the K-th value are in the K by
//      lowest index first: when not all of them fit, a scan over the row finds the index of the last one that does.
//   3. The memories of the sample are given sorted by value id (slot order); a group is a run of equal ids.  The thread
//      whose slot starts a run walks it in slot order under a running maximum, subtracts the normaliser, merges with the
//      id's vocabulary entry where step 2 admits it, and the workgroup takes the arg-max: larger value first, then the
//      top-1 before any group, then the lower id (= the earlier run).
//   4. Thread 0 updates the state.  A sample that is done is fed end_id and changes nothing else.  With `live` (the
//      early exit of ptgnn_amd_greedy_step_live_f32) a sample that is not done after the step adds 1 to live[step]: an
//      integer atomic, so the sum does not depend on the order of arrival.
// Exact ties are the one place where the reference leaves the outcome open (to torch.topk and to dict order); here they
// are decided as above.  No float atomics, fixed fold orders: two launches give the same bits.
#include "decode_common.h"

namespace ptgnn_amd {
namespace {

// the order of the row's top-1: the larger value, the lower column among equals
__device__ __forceinline__ bool first_top(const Cand &a, const Cand &b) { return a.v > b.v || (a.v == b.v && a.id < b.id); }

__global__ __launch_bounds__(kDecThreads) void k_decode_step(
    const float *__restrict__ scores, int64_t ld, const float *__restrict__ bias, const float *__restrict__ copy,
    const float *__restrict__ total_copy, const int32_t *__restrict__ slot_memory, const int32_t *__restrict__ rowptr,
    const int64_t *__restrict__ slot_ids, int64_t num_memories, int vocab, int top_k, int64_t unk_id, int64_t end_id,
    int step, int max_steps, int32_t *__restrict__ done, int64_t *__restrict__ lengths, float *__restrict__ logprobs,
    int64_t *__restrict__ tokens, int64_t *__restrict__ next_tokens, int32_t *__restrict__ bad,
    int32_t *__restrict__ live) {
  __shared__ MaxSum s_ms[kDecWaves];
  __shared__ Cand s_cand[kDecWaves];
  __shared__ RadixSelect s_select;
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  if (done[b]) {                                             // workgroup-uniform
    if (t == 0) next_tokens[b] = end_id;
    return;
  }
  const float *row = scores + (int64_t)b * ld;

  // 1. normaliser and top-1
  MaxSum a{-INFINITY, 0.0f};
  Cand best{-INFINITY, -1, (int64_t)INT32_MAX};
  for (int c = t; c < vocab; c += kDecThreads) {             // ascending columns: the first of equal values is kept
    const float v = score_at(row, bias, c);
    push(a, v);
    if (v > best.v || best.id == INT32_MAX) best.v = v, best.id = c;
  }
  a = wave_fold(a, combine);
  best = wave_fold(best, first_by(first_top));
  leader_store(best, s_cand);
  a = waves_in_order<kDecWaves>(a, s_ms, combine);           // its barrier is s_cand's too
  best = fold_in_order<kDecWaves>(s_cand, first_by(first_top));
  a = combine(a, MaxSum{total_copy[b], 1.0f});               // -inf: (max, sum) unchanged, bit for bit
  const float top = a.m, log_sum = a.m == -INFINITY ? 0.0f : logf(a.s);
  best.v = (best.v - top) - log_sum;
  best.rank = -1;
  __syncthreads();                                           // s_cand is written again in step 3

  // 2. the K-th largest key of the row; cut = the highest index with that key that is still one of the K
  const bool all_in = top_k >= vocab;
  uint32_t kth = 0;
  int cut = INT32_MAX;
  if (!all_in) s_select.select(row, bias, vocab, top_k, kth, cut);   // csrc/decode_common.h

  // 3. the sample's value groups
  const int lo = rowptr[b], hi = rowptr[b + 1];
  Cand mine{-INFINITY, INT32_MAX, 0};
  int wrong = 0;
  for (int s = lo + t; s < hi; s += kDecThreads) {
    const int64_t g = slot_ids[s];
    if (s > lo && slot_ids[s - 1] == g) continue;            // not the start of a run
    MaxSum r{-INFINITY, 0.0f};
    for (int q = s; q < hi && slot_ids[q] == g; ++q) {       // slot order
      int64_t i = slot_memory[q];
      if (i < 0 || i >= num_memories) ++wrong, i = 0;
      push(r, copy[i]);
    }
    float v = r.m == -INFINITY ? -INFINITY : ((r.m - top) + logf(r.s)) - log_sum;
    if (g < 0) {
      ++wrong;
    } else if (g < vocab) {
      const float sv = score_at(row, bias, (int)g);
      const uint32_t key = order_key(sv);
      if (all_in || key > kth || (key == kth && (int)g <= cut)) v = log_add_exp((sv - top) - log_sum, v);
    }
    const Cand c{v, s, g < 0 ? 0 : g};
    if (better(c, mine)) mine = c;
  }
  if (wrong && bad) atomicAdd(bad, wrong);
  if (t == 0 && better(best, mine)) mine = best;             // -inf everywhere: the top-1
  mine = wave_fold(mine, first_by(better));
  mine = waves_in_order<kDecWaves>(mine, s_cand, first_by(better), t == 0);   // thread 0 alone folds the waves
  if (t != 0) return;

  // 4. the state
  if (!(mine.rank < INT32_MAX)) mine = best;                 // nothing compared greater (nan scores): the top-1
  logprobs[b] += mine.v;
  if (mine.id == end_id) {
    done[b] = 1;
  } else {
    if (step < max_steps) tokens[(int64_t)b * max_steps + step] = mine.id;
    lengths[b] += 1;
    if (live) atomicAdd(live + step, 1);
  }
  next_tokens[b] = mine.id < vocab ? mine.id : unk_id;
}

// what the two entries share: the checks, then the one launch
int decode_step_launch(const float *scores, int64_t ld, const float *bias, const float *copy_scores, const float *total_copy,
                       const int32_t *slot_memory, const int32_t *rowptr, const int64_t *slot_ids, int64_t num_samples,
                       int64_t num_memories, int32_t vocab, int32_t top_k, int64_t unk_id, int64_t end_id, int32_t step,
                       int32_t max_steps, int32_t *done, int64_t *lengths, float *logprobs, int64_t *tokens,
                       int64_t *next_tokens, int32_t *bad, int32_t *live, bool needs_live, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && num_memories >= 0 && vocab >= 1 && top_k >= 1, PTGNN_AMD_EINVAL,
                "decode_step: bad sizes (samples %lld, memories %lld, vocab %d, top_k %d)", (long long)num_samples,
                (long long)num_memories, vocab, top_k);
  PTGNN_REQUIRE(ld >= vocab, PTGNN_AMD_EINVAL, "decode_step: leading dimension %lld < vocab %d", (long long)ld, vocab);
  PTGNN_REQUIRE(step >= 0 && step < max_steps, PTGNN_AMD_EINVAL, "decode_step: step %d outside [0, %d)", step, max_steps);
  PTGNN_REQUIRE(unk_id >= 0 && unk_id < vocab && end_id >= 0 && end_id < vocab, PTGNN_AMD_EINVAL,
                "decode_step: unk_id %lld / end_id %lld outside the vocabulary of %d", (long long)unk_id,
                (long long)end_id, vocab);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_samples < lim && num_memories < lim && vocab < lim - kDecThreads &&
                    num_samples <= (lim - 1) / max_steps,
                PTGNN_AMD_EUNSUPPORTED, "decode_step: too many samples / memories / columns");
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(scores && total_copy && rowptr && done && lengths && logprobs && tokens && next_tokens &&
                    (num_memories == 0 || (copy_scores && slot_memory && slot_ids)),
                PTGNN_AMD_EINVAL, "decode_step: null pointer");
  PTGNN_REQUIRE(live || !needs_live, PTGNN_AMD_EINVAL, "decode_step: null live counter");
  k_decode_step<<<(unsigned)num_samples, kDecThreads, 0, (hipStream_t)stream_>>>(
      scores, ld, bias, copy_scores, total_copy, slot_memory, rowptr, slot_ids, num_memories, vocab, top_k, unk_id, end_id,
      step, max_steps, done, lengths, logprobs, tokens, next_tokens, bad, live);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_DECODE_STEP);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" size_t ptgnn_amd_decode_step_workspace_bytes(int64_t num_samples, int32_t vocab, int32_t top_k) {
  (void)num_samples, (void)vocab, (void)top_k;
  return 0;     // a sample's partial results live in LDS and registers of its one workgroup
}

extern "C" int ptgnn_amd_decode_step_f32(const float *scores, int64_t ld, const float *bias, const float *copy_scores,
                                         const float *total_copy, const int32_t *slot_memory, const int32_t *rowptr,
                                         const int64_t *slot_ids, int64_t num_samples, int64_t num_memories,
                                         int32_t vocab, int32_t top_k, int64_t unk_id, int64_t end_id, int32_t step,
                                         int32_t max_steps, int32_t *done, int64_t *lengths, float *logprobs,
                                         int64_t *tokens, int64_t *next_tokens, int32_t *bad, void *workspace,
                                         size_t workspace_bytes, void *stream_) {
  (void)workspace, (void)workspace_bytes;
  return decode_step_launch(scores, ld, bias, copy_scores, total_copy, slot_memory, rowptr, slot_ids, num_samples,
                            num_memories, vocab, top_k, unk_id, end_id, step, max_steps, done, lengths, logprobs, tokens,
                            next_tokens, bad, nullptr, false, stream_);
}

extern "C" int ptgnn_amd_greedy_step_live_f32(const float *scores, int64_t ld, const float *bias, const float *copy_scores,
                                              const float *total_copy, const int32_t *slot_memory, const int32_t *rowptr,
                                              const int64_t *slot_ids, int64_t num_samples, int64_t num_memories,
                                              int32_t vocab, int32_t top_k, int64_t unk_id, int64_t end_id, int32_t step,
                                              int32_t max_steps, int32_t *done, int64_t *lengths, float *logprobs,
                                              int64_t *tokens, int64_t *next_tokens, int32_t *live, int32_t *bad,
                                              void *workspace, size_t workspace_bytes, void *stream_) {
  (void)workspace, (void)workspace_bytes;
  return decode_step_launch(scores, ld, bias, copy_scores, total_copy, slot_memory, rowptr, slot_ids, num_samples,
                            num_memories, vocab, top_k, unk_id, end_id, step, max_steps, done, lengths, logprobs, tokens,
                            next_tokens, bad, live, true, stream_);
}
