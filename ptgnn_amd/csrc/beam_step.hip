// One step of the copying decoder's beam search: k_decode_step (csrc/decode_step.hip) widened from the top-1 of a sample
// to the W best continuations of a sample's W hypotheses.  From the RAW vocabulary scores [B W, V] (row b W + j: slot j of
// sample b) and the copy scores [I, W] of the step straight to the new slots: their scores, their parents, the next input
// tokens and the reordered token histories.  Neither the [B W, V] log-probabilities nor a ranking of them exists, nothing
// visits the host.
//
// A live slot j of sample b has the entries of greedy decoding's dictionary, built from ITS row and ITS copy scores: the
// K = top_k largest s[v] - norm, merged with the sample's value groups (onto the vocabulary entry where the id is one of
// the K, onto -inf elsewhere).  Entry e is the candidate (parent j, id e, score[j] + logprob(e)); a finished slot is its
// own single candidate.  The W candidates of the sample that come first by
//     higher score; lower parent; inside a parent the ids of its W best vocabulary columns before its other entries;
//     lower id
// are the new slots 0 .. W - 1.  What a parent can contribute lies in the union of its W best vocabulary entries (each
// with its group merged in where it has one) and the sample's groups on other ids: any other entry is a plain vocabulary
// entry outside the W best, and those W come before it.  So a parent needs the normaliser, its W best columns and the
// K-th threshold with its tie cut -- steps 1 to 3 of k_decode_step with the arg-max widened to the W first.
//
// Two kernels, a workspace between them, no hand-off between workgroups inside a launch:
//   k_beam_candidates  one workgroup of kDecThreads threads per (sample, parent).  The normaliser in one pass over the
//       row (the fold of k_decode_step: W = 1 gives its bits); the W-th and the K-th largest key by the radix select of
//       csrc/decode_common.h, the row re-read from L2; the W best columns collected into LDS; the sample's groups walked
//       as in k_decode_step with the parent's column of the copy scores, a group on one of the W best ids REPLACING that
//       entry; then W rounds of a workgroup arg-max, each taking the first entry after the previous round's in the order
//       above, write the parent's W candidates (score, id, tie class).  A finished or -inf parent writes its candidates
//       without reading its row.
//   k_beam_select  one wave per sample: each of the <= W W candidates counts those in front of it; the first W write the
//       state out -- the token history of the chosen parent copied with the new id appended -- and next_tokens and
//       parent_rows.  It also counts the slots that had to be clamped, once per call.
// Exact fp32, integer atomics only, fixed fold orders: two calls give the same bits.
//
// The finishing route (ptgnn_amd_search_step_links_f32, ptgnn_amd_search_backtrack) is the same step with three
// differences, all in the selection kernel, which is ONE body with a compile-time switch (k_beam_select<kLinks>):
//   * candidates are placed by key = score * key_scale[lengths_in[parent] + 1], a table the host made (GNMT length
//     normalisation; no powf and no division here).  Every candidate of a parent has the same scale, so the order inside
//     a parent is the order of the raw sums and k_beam_candidates runs unchanged.  The state keeps the raw sums.
//   * a slot writes the pair links[step, b, slot] = (appended id or -1, parent slot), 8 bytes, where k_beam_select<false>
//     copies a history of 8 max_steps bytes; k_beam_backtrack walks the pairs once per call, one thread per final slot: a
//     chain of `steps_run` DEPENDENT 8-byte loads per thread, B W threads, one launch a call.
//   * the sample's number of live output slots is added to live[step]: one integer atomic per sample.
#include "decode_common.h"

namespace ptgnn_amd {
namespace {

constexpr int kBeamMax = 8;              // the head limit of the fused attention pool
constexpr int kNoCand = INT32_MAX;       // tie class of a candidate place that holds nothing

// the order of the candidates of one parent: `rank` is the tie class (0: the id is one of the parent's W best columns)
__device__ __forceinline__ bool before(const Cand &a, const Cand &b) {
  return a.v > b.v || (a.v == b.v && (a.rank < b.rank || (a.rank == b.rank && a.id < b.id)));
}

__global__ __launch_bounds__(kDecThreads) void k_beam_candidates(
    const float *__restrict__ scores, int64_t ld, const float *__restrict__ bias, const float *__restrict__ copy,
    const float *__restrict__ total_copy, const int32_t *__restrict__ slot_memory, const int32_t *__restrict__ rowptr,
    const int64_t *__restrict__ slot_ids, int64_t num_memories, int vocab, int top_k, int W,
    const float *__restrict__ score_in, const int32_t *__restrict__ done_in, float *__restrict__ group_value,
    float *__restrict__ cand_score, int64_t *__restrict__ cand_id, int32_t *__restrict__ cand_class) {
  __shared__ MaxSum s_ms[kDecWaves];
  __shared__ Cand s_cand[kDecWaves];
  __shared__ RadixSelect s_select;
  __shared__ int s_top_id[kBeamMax];
  __shared__ float s_top_v[kBeamMax];
  __shared__ int s_count;
  const int b = blockIdx.x / W, j = blockIdx.x % W;
  const int t = threadIdx.x;
  const int64_t r = blockIdx.x;                              // b W + j
  float *out_v = cand_score + r * W;
  int64_t *out_id = cand_id + r * W;
  int32_t *out_class = cand_class + r * W;
  const float base = score_in[r];
  if (done_in[r]) {                                          // workgroup-uniform: itself, nothing appended
    if (t < W) out_v[t] = t == 0 ? base : -INFINITY, out_id[t] = -1, out_class[t] = t == 0 ? 0 : kNoCand;
    return;
  }
  if (!(base > -INFINITY)) {                                 // every candidate is -inf: behind all finite ones
    if (t < W) out_v[t] = -INFINITY, out_id[t] = t, out_class[t] = 0;
    return;
  }
  const float *row = scores + r * ld;

  // 1. the normaliser (k_decode_step's fold)
  MaxSum a{-INFINITY, 0.0f};
  for (int c = t; c < vocab; c += kDecThreads) push(a, score_at(row, bias, c));
  if (t == 0) s_count = 0;
  a = waves_in_order<kDecWaves>(wave_fold(a, combine), s_ms, combine);
  a = combine(a, MaxSum{total_copy[r], 1.0f});
  const float top = a.m, log_sum = a.m == -INFINITY ? 0.0f : logf(a.s);

  // 2. the W best columns, and the K-th largest key with its tie cut
  const bool all_top = W >= vocab, all_in = top_k >= vocab;
  uint32_t kth_w = 0, kth = 0;
  int cut_w = INT32_MAX, cut = INT32_MAX;
  if (!all_top) s_select.select(row, bias, vocab, W, kth_w, cut_w);
  if (!all_in) {
    if (top_k == W) kth = kth_w, cut = cut_w;
    else s_select.select(row, bias, vocab, top_k, kth, cut);
  }
  for (int c = t; c < vocab; c += kDecThreads) {
    const float v = score_at(row, bias, c);
    const uint32_t key = order_key(v);
    if (all_top || key > kth_w || (key == kth_w && c <= cut_w)) {
      const int p = atomicAdd(&s_count, 1);                  // the place is arbitrary, the set is not; rounds order it
      if (p < kBeamMax) s_top_id[p] = c, s_top_v[p] = base + ((v - top) - log_sum);
    }
  }
  __syncthreads();
  const int num_top = s_count < W ? s_count : W;             // W, unless nan scores kept the select from counting

  // 3. the sample's value groups with this parent's copy scores
  const int lo = rowptr[b], hi = rowptr[b + 1];
  float *value_of = group_value + (int64_t)j * num_memories;
  for (int s = lo + t; s < hi; s += kDecThreads) {
    const int64_t g = slot_ids[s];
    if (s > lo && slot_ids[s - 1] == g) continue;            // not the start of a run
    MaxSum run{-INFINITY, 0.0f};
    for (int q = s; q < hi && slot_ids[q] == g; ++q) {       // slot order
      int64_t i = slot_memory[q];
      if (i < 0 || i >= num_memories) i = 0;                 // counted by k_beam_select
      push(run, copy[i * W + j]);
    }
    float v = run.m == -INFINITY ? -INFINITY : ((run.m - top) + logf(run.s)) - log_sum;
    int place = -1;
    if (g >= 0 && g < vocab) {
      const float sv = score_at(row, bias, (int)g);
      const uint32_t key = order_key(sv);
      if (all_in || key > kth || (key == kth && (int)g <= cut)) v = log_add_exp((sv - top) - log_sum, v);
      for (int k = 0; k < num_top; ++k)
        if (s_top_id[k] == (int)g) place = k;
    }
    v = base + v;
    if (place >= 0) s_top_v[place] = v;                      // one run per id: no other thread writes this place
    value_of[s] = place >= 0 ? NAN : v;                      // nan: no entry of its own, it never compares first
  }
  __syncthreads();

  // 4. W rounds: the first entry after the previous round's
  Cand prev{0.0f, 0, 0};
  for (int k = 0; k < W; ++k) {
    Cand mine{-INFINITY, kNoCand, 0};
    if (t < num_top) {
      const Cand c{s_top_v[t], 0, (int64_t)s_top_id[t]};
      if ((k == 0 || before(prev, c)) && before(c, mine)) mine = c;
    }
    for (int s = lo + t; s < hi; s += kDecThreads) {
      const int64_t g = slot_ids[s];
      if (s > lo && slot_ids[s - 1] == g) continue;
      const Cand c{value_of[s], 1, g < 0 ? 0 : g};
      if ((k == 0 || before(prev, c)) && before(c, mine)) mine = c;
    }
    mine = waves_in_order<kDecWaves>(wave_fold(mine, first_by(before)), s_cand, first_by(before));
    __syncthreads();                                         // s_cand is written again in the next round
    if (t == 0) out_v[k] = mine.v, out_id[k] = mine.id, out_class[k] = mine.rank;
    if (mine.rank == kNoCand) {                              // workgroup-uniform; nothing is left (nan scores)
      if (t > k && t < W) out_v[t] = -INFINITY, out_id[t] = 0, out_class[t] = kNoCand;
      break;
    }
    prev = mine;
  }
}

// kLinks = false: ptgnn_amd_beam_step_f32 (place by score, copy the histories; key_scale / links / live are not read).
// kLinks = true: the finishing route (place by key, write the back-pointer pairs, count the live slots; tokens_in /
// tokens_out are not read).
template <bool kLinks>
__global__ __launch_bounds__(kWave) void k_beam_select(
    const float *__restrict__ cand_score, const int64_t *__restrict__ cand_id, const int32_t *__restrict__ cand_class,
    const int32_t *__restrict__ slot_memory, const int32_t *__restrict__ rowptr, const int64_t *__restrict__ slot_ids,
    int64_t num_memories, int vocab, int W, int64_t unk_id, int64_t end_id, int step, int max_steps,
    const float *__restrict__ score_in, const int32_t *__restrict__ done_in, const int64_t *__restrict__ lengths_in,
    const int64_t *__restrict__ tokens_in, float *__restrict__ score_out, int32_t *__restrict__ done_out,
    int64_t *__restrict__ lengths_out, int64_t *__restrict__ tokens_out, int64_t *__restrict__ next_tokens,
    int64_t *__restrict__ parent_rows, int32_t *__restrict__ bad, const float *__restrict__ key_scale,
    int32_t *__restrict__ links, int32_t *__restrict__ live, int64_t num_samples) {
  __shared__ float s_v[kBeamMax * kBeamMax];
  __shared__ float s_key[kBeamMax * kBeamMax];                // what the candidates are placed by
  __shared__ int s_class[kBeamMax * kBeamMax];
  __shared__ int64_t s_id[kBeamMax * kBeamMax];
  __shared__ int s_pick[kBeamMax];
  const int b = blockIdx.x, l = threadIdx.x, n = W * W;
  const int64_t first = (int64_t)b * W;                      // the sample's first row
  if (l < n) {
    const float v = cand_score[first * W + l];
    s_v[l] = v, s_id[l] = cand_id[first * W + l], s_class[l] = cand_class[first * W + l];
    if constexpr (kLinks) {                                  // the parent's scale: -inf stays -inf, nan stays nan
      int64_t decisions = lengths_in[first + l / W] + 1;
      decisions = decisions < 0 ? 0 : (decisions > max_steps ? max_steps : decisions);
      s_key[l] = v * key_scale[decisions];
    } else {
      s_key[l] = v;
    }
  }
  if (l < W) s_pick[l] = -1;
  __syncthreads();
  if (l < n && s_class[l] != kNoCand) {                      // candidate l = parent l / W, its (l % W)-th
    const float v = s_key[l];
    const int parent = l / W, cls = s_class[l];
    const int64_t id = s_id[l];
    int place = 0;
    for (int m = 0; m < n; ++m) {
      if (m == l || s_class[m] == kNoCand) continue;
      const float u = s_key[m];
      const int p = m / W;
      if (u > v || (u == v && (p < parent || (p == parent && (s_class[m] < cls || (s_class[m] == cls && s_id[m] < id))))))
        ++place;
    }
    if (place < W) s_pick[place] = l;
  }
  __syncthreads();
  int alive = 0;
  if (l < W) {                                               // slot l of the sample
    const int pick = s_pick[l];
    const int64_t out = first + l, from = first + (pick < 0 ? l : pick / W);
    const bool finished = done_in[from] != 0 || pick < 0;    // pick < 0: nan scores left the place empty; carried over
    const int64_t id = pick < 0 ? end_id : s_id[pick];
    const bool ends = !finished && id == end_id;
    score_out[out] = pick < 0 ? score_in[from] : s_v[pick];
    done_out[out] = finished || ends ? 1 : 0;
    lengths_out[out] = lengths_in[from] + (finished || ends ? 0 : 1);
    next_tokens[out] = finished ? end_id : (id < vocab ? id : unk_id);
    parent_rows[out] = from;
    if constexpr (kLinks) {                                  // what the slot appends and where it came from
      int32_t *pair = links + (((int64_t)step * num_samples + b) * W + l) * 2;
      pair[0] = finished || ends ? -1 : (int32_t)id;
      pair[1] = (int32_t)(from - first);
      alive = finished || ends ? 0 : 1;
    }
  }
  if constexpr (kLinks) {
    const int count = __popcll(__ballot(alive));             // the workgroup is one wave
    if (live && l == 0 && count) atomicAdd(live + step, count);
  } else {
    for (int p = 0; p < W; ++p) {                            // the histories, each with what its slot appends
      const int pick = s_pick[p];
      const int64_t out = first + p, from = first + (pick < 0 ? p : pick / W);
      const bool appends = pick >= 0 && done_in[from] == 0 && s_id[pick] != end_id;
      for (int c = l; c < max_steps; c += kWave)
        tokens_out[out * max_steps + c] = appends && c == step ? s_id[pick] : tokens_in[from * max_steps + c];
    }
  }
  if (bad) {                                                 // what k_beam_candidates clamped, counted once
    int wrong = 0;
    for (int s = rowptr[b] + l; s < rowptr[b + 1]; s += kWave) {
      const int64_t i = slot_memory[s];
      if (i < 0 || i >= num_memories) ++wrong;
      if (slot_ids[s] < 0) ++wrong;
    }
    if (wrong) atomicAdd(bad, wrong);
  }
}

constexpr int kBacktrackThreads = 256;

// One thread per final slot (b, w): from the last step that ran back to step 0 through the back-pointer pairs.  A token
// appended at step s sits at column s (a live hypothesis has appended at every earlier step), so there is no length
// arithmetic; the columns from steps_run on are -1, so the caller allocates `tokens` without a fill.
__global__ __launch_bounds__(kBacktrackThreads) void k_beam_backtrack(
    const int32_t *__restrict__ links, int64_t num_samples, int W, int steps_run, int max_steps,
    int64_t *__restrict__ tokens) {
  const int64_t i = (int64_t)blockIdx.x * kBacktrackThreads + threadIdx.x;
  if (i >= num_samples * W) return;
  const int64_t b = i / W;
  int slot = (int)(i % W);
  int64_t *row = tokens + i * max_steps;
  for (int c = steps_run; c < max_steps; ++c) row[c] = -1;
  for (int s = steps_run - 1; s >= 0; --s) {
    const int2 pair = *reinterpret_cast<const int2 *>(links + (((int64_t)s * num_samples + b) * W + slot) * 2);
    row[s] = pair.x;
    slot = pair.y < 0 ? 0 : (pair.y >= W ? W - 1 : pair.y);  // the step kernel wrote a slot of the sample
  }
}

struct BeamWorkspace {
  size_t group_value, cand_score, cand_id, cand_class, total;
};

BeamWorkspace beam_workspace(int64_t num_samples, int64_t num_memories, int beam_width) {
  Carve c;
  BeamWorkspace w;
  const size_t cands = (size_t)num_samples * beam_width * beam_width;
  w.group_value = c.take((size_t)num_memories * beam_width * sizeof(float));
  w.cand_score = c.take(cands * sizeof(float));
  w.cand_id = c.take(cands * sizeof(int64_t));
  w.cand_class = c.take(cands * sizeof(int32_t));
  w.total = c.off;
  return w;
}

// 0 when the sizes are fine; sets the error text
int beam_sizes_check(int64_t num_samples, int64_t num_memories, int32_t vocab, int32_t top_k, int32_t beam_width,
                     int32_t max_steps) {
  PTGNN_REQUIRE(num_samples >= 0 && num_memories >= 0 && vocab >= 1 && top_k >= 1, PTGNN_AMD_EINVAL,
                "beam_step: bad sizes (samples %lld, memories %lld, vocab %d, top_k %d)", (long long)num_samples,
                (long long)num_memories, vocab, top_k);
  PTGNN_REQUIRE(beam_width >= 1 && beam_width <= kBeamMax && beam_width <= top_k && beam_width <= vocab, PTGNN_AMD_EINVAL,
                "beam_step: beam_width %d outside [1, min(%d, top_k %d, vocab %d)]", beam_width, kBeamMax, top_k, vocab);
  PTGNN_REQUIRE(max_steps >= 1, PTGNN_AMD_EINVAL, "beam_step: max_steps %d < 1", max_steps);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_samples <= (lim - 1) / ((int64_t)beam_width * beam_width) && num_memories <= (lim - 1) / beam_width &&
                    vocab < lim - kDecThreads && num_samples * beam_width <= (lim - 1) / max_steps,
                PTGNN_AMD_EUNSUPPORTED, "beam_step: too many samples / memories / columns");
  return PTGNN_AMD_OK;
}

// the checks the two step entries share, in the order ptgnn_amd_beam_step_f32 makes them
int beam_step_check(int64_t ld, int64_t num_samples, int64_t num_memories, int32_t vocab, int32_t top_k, int32_t beam_width,
                    int64_t unk_id, int64_t end_id, int32_t step, int32_t max_steps) {
  PTGNN_REQUIRE(step >= 0 && step < max_steps, PTGNN_AMD_EINVAL, "beam_step: step %d outside [0, %d)", step, max_steps);
  if (const int rc = beam_sizes_check(num_samples, num_memories, vocab, top_k, beam_width, max_steps)) return rc;
  PTGNN_REQUIRE(ld >= vocab, PTGNN_AMD_EINVAL, "beam_step: leading dimension %lld < vocab %d", (long long)ld, vocab);
  PTGNN_REQUIRE(unk_id >= 0 && unk_id < vocab && end_id >= 0 && end_id < vocab, PTGNN_AMD_EINVAL,
                "beam_step: unk_id %lld / end_id %lld outside the vocabulary of %d", (long long)unk_id, (long long)end_id,
                vocab);
  return PTGNN_AMD_OK;
}

// 0 when the back-pointer pairs [max_steps, B, W, 2] can be indexed; sets the error text
int links_sizes_check(const char *who, int64_t num_samples, int32_t beam_width, int32_t max_steps) {
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_samples * beam_width <= (lim - 1) / 2 / max_steps, PTGNN_AMD_EUNSUPPORTED,
                "%s: too many samples / steps for the back-pointer pairs", who);
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" size_t ptgnn_amd_beam_step_workspace_bytes(int64_t num_samples, int64_t num_memories, int32_t vocab,
                                                      int32_t top_k, int32_t beam_width) {
  if (num_samples <= 0 || beam_sizes_check(num_samples, num_memories, vocab, top_k, beam_width, 1) != PTGNN_AMD_OK) return 0;
  return beam_workspace(num_samples, num_memories, beam_width).total;
}


extern "C" int ptgnn_amd_beam_step_f32(const float *scores, int64_t ld, const float *bias, const float *copy_scores,
                                       const float *total_copy, const int32_t *slot_memory, const int32_t *rowptr,
                                       const int64_t *slot_ids, int64_t num_samples, int64_t num_memories, int32_t vocab,
                                       int32_t top_k, int32_t beam_width, int64_t unk_id, int64_t end_id, int32_t step,
                                       int32_t max_steps, const float *beam_scores_in, const int32_t *done_in,
                                       const int64_t *lengths_in, const int64_t *tokens_in, float *beam_scores_out,
                                       int32_t *done_out, int64_t *lengths_out, int64_t *tokens_out, int64_t *next_tokens,
                                       int64_t *parent_rows, int32_t *bad, void *workspace, size_t workspace_bytes,
                                       void *stream_) {
  if (const int rc = beam_step_check(ld, num_samples, num_memories, vocab, top_k, beam_width, unk_id, end_id, step, max_steps))
    return rc;
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(scores && total_copy && rowptr && beam_scores_in && done_in && lengths_in && tokens_in && beam_scores_out &&
                    done_out && lengths_out && tokens_out && next_tokens && parent_rows &&
                    (num_memories == 0 || (copy_scores && slot_memory && slot_ids)),
                PTGNN_AMD_EINVAL, "beam_step: null pointer");
  const BeamWorkspace w = beam_workspace(num_samples, num_memories, beam_width);
  PTGNN_REQUIRE(workspace && workspace_bytes >= w.total, PTGNN_AMD_EINVAL, "beam_step: workspace of %zu bytes, need %zu",
                workspace_bytes, w.total);
  float *group_value = carved<float>(workspace, w.group_value);
  float *cand_score = carved<float>(workspace, w.cand_score);
  int64_t *cand_id = carved<int64_t>(workspace, w.cand_id);
  int32_t *cand_class = carved<int32_t>(workspace, w.cand_class);
  hipStream_t st = (hipStream_t)stream_;
  k_beam_candidates<<<(unsigned)(num_samples * beam_width), kDecThreads, 0, st>>>(
      scores, ld, bias, copy_scores, total_copy, slot_memory, rowptr, slot_ids, num_memories, vocab, top_k, beam_width,
      beam_scores_in, done_in, group_value, cand_score, cand_id, cand_class);
  PTGNN_LAUNCH_CHECK();
  k_beam_select<false><<<(unsigned)num_samples, kWave, 0, st>>>(
      cand_score, cand_id, cand_class, slot_memory, rowptr, slot_ids, num_memories, vocab, beam_width, unk_id, end_id, step,
      max_steps, beam_scores_in, done_in, lengths_in, tokens_in, beam_scores_out, done_out, lengths_out, tokens_out,
      next_tokens, parent_rows, bad, nullptr, nullptr, nullptr, num_samples);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BEAM_STEP);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_search_step_links_f32(const float *scores, int64_t ld, const float *bias, const float *copy_scores,
                                               const float *total_copy, const int32_t *slot_memory, const int32_t *rowptr,
                                               const int64_t *slot_ids, int64_t num_samples, int64_t num_memories,
                                               int32_t vocab, int32_t top_k, int32_t beam_width, int64_t unk_id,
                                               int64_t end_id, int32_t step, int32_t max_steps, const float *key_scale,
                                               const float *beam_scores_in, const int32_t *done_in,
                                               const int64_t *lengths_in, float *beam_scores_out, int32_t *done_out,
                                               int64_t *lengths_out, int64_t *next_tokens, int64_t *parent_rows,
                                               int32_t *links, int32_t *live, int32_t *bad, void *workspace,
                                               size_t workspace_bytes, void *stream_) {
  if (const int rc = beam_step_check(ld, num_samples, num_memories, vocab, top_k, beam_width, unk_id, end_id, step, max_steps))
    return rc;
  if (const int rc = links_sizes_check("beam_step_links", num_samples, beam_width, max_steps)) return rc;
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(scores && total_copy && rowptr && key_scale && beam_scores_in && done_in && lengths_in && beam_scores_out &&
                    done_out && lengths_out && next_tokens && parent_rows && links &&
                    (num_memories == 0 || (copy_scores && slot_memory && slot_ids)),
                PTGNN_AMD_EINVAL, "beam_step_links: null pointer");
  const BeamWorkspace w = beam_workspace(num_samples, num_memories, beam_width);
  PTGNN_REQUIRE(workspace && workspace_bytes >= w.total, PTGNN_AMD_EINVAL,
                "beam_step_links: workspace of %zu bytes, need %zu", workspace_bytes, w.total);
  float *group_value = carved<float>(workspace, w.group_value);
  float *cand_score = carved<float>(workspace, w.cand_score);
  int64_t *cand_id = carved<int64_t>(workspace, w.cand_id);
  int32_t *cand_class = carved<int32_t>(workspace, w.cand_class);
  hipStream_t st = (hipStream_t)stream_;
  k_beam_candidates<<<(unsigned)(num_samples * beam_width), kDecThreads, 0, st>>>(
      scores, ld, bias, copy_scores, total_copy, slot_memory, rowptr, slot_ids, num_memories, vocab, top_k, beam_width,
      beam_scores_in, done_in, group_value, cand_score, cand_id, cand_class);
  PTGNN_LAUNCH_CHECK();
  k_beam_select<true><<<(unsigned)num_samples, kWave, 0, st>>>(
      cand_score, cand_id, cand_class, slot_memory, rowptr, slot_ids, num_memories, vocab, beam_width, unk_id, end_id, step,
      max_steps, beam_scores_in, done_in, lengths_in, nullptr, beam_scores_out, done_out, lengths_out, nullptr, next_tokens,
      parent_rows, bad, key_scale, links, live, num_samples);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BEAM_STEP_LINKS);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_search_backtrack(const int32_t *links, int64_t num_samples, int32_t beam_width, int32_t steps_run,
                                          int32_t max_steps, int64_t *tokens, void *stream_) {
  PTGNN_REQUIRE(num_samples >= 0 && beam_width >= 1 && beam_width <= kBeamMax && max_steps >= 1, PTGNN_AMD_EINVAL,
                "beam_backtrack: bad sizes (samples %lld, beam_width %d, max_steps %d)", (long long)num_samples, beam_width,
                max_steps);
  PTGNN_REQUIRE(steps_run >= 0 && steps_run <= max_steps, PTGNN_AMD_EINVAL, "beam_backtrack: steps_run %d outside [0, %d]",
                steps_run, max_steps);
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(num_samples <= (lim - 1) / beam_width, PTGNN_AMD_EUNSUPPORTED, "beam_backtrack: too many samples");
  if (const int rc = links_sizes_check("beam_backtrack", num_samples, beam_width, max_steps)) return rc;
  if (num_samples == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(links && tokens, PTGNN_AMD_EINVAL, "beam_backtrack: null pointer");
  const int64_t slots = num_samples * beam_width;
  k_beam_backtrack<<<(unsigned)((slots + kBacktrackThreads - 1) / kBacktrackThreads), kBacktrackThreads, 0,
                     (hipStream_t)stream_>>>(links, num_samples, beam_width, steps_run, max_steps, tokens);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BEAM_BACKTRACK);
  return PTGNN_AMD_OK;
}
