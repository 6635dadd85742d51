// Thread-local error message + version for libptgnn_amd.
#include <stdarg.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <unordered_map>

#include "common.h"

namespace ptgnn_amd {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// Launch counters of the GEMM kernel families (ptgnn_amd_launch_count): which kernel a call was dispatched to is a
// shape / size / mode decision the tests assert on (a parity test that silently ran the tile kernel pins nothing about
// the streaming one).  Relaxed atomics on the host side of a launch; never read by the library itself.
static std::atomic<int64_t> g_launches[PTGNN_AMD_KERNEL_COUNT_];
static std::atomic<int64_t> g_agg_launches[PTGNN_AMD_KERNEL_AGG_END_ - PTGNN_AMD_KERNEL_AGG_FIRST_];
static std::atomic<int64_t> g_char_launches[PTGNN_AMD_KERNEL_CHAR_END_ - PTGNN_AMD_KERNEL_CHAR_FIRST_];
static std::atomic<int64_t> g_head_launches[PTGNN_AMD_KERNEL_HEAD_END_ - PTGNN_AMD_KERNEL_HEAD_FIRST_];
static std::atomic<int64_t> g_seq_launches[PTGNN_AMD_KERNEL_SEQ_END_ - PTGNN_AMD_KERNEL_SEQ_FIRST_];
static std::atomic<int64_t> g_decode_launches[PTGNN_AMD_KERNEL_DECODE_END_ - PTGNN_AMD_KERNEL_DECODE_FIRST_];
static std::atomic<int64_t> g_beam_launches[PTGNN_AMD_KERNEL_BEAM_END_ - PTGNN_AMD_KERNEL_BEAM_FIRST_];
static std::atomic<int64_t> g_half_launches[PTGNN_AMD_KERNEL_HALF_END_ - PTGNN_AMD_KERNEL_HALF_FIRST_];
static std::atomic<int64_t> g_edge16_launches[PTGNN_AMD_KERNEL_EDGE16_END_ - PTGNN_AMD_KERNEL_EDGE16_FIRST_];
static std::atomic<int64_t> g_half_train_launches[PTGNN_AMD_KERNEL_HALF_TRAIN_END_ - PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_];
static std::atomic<int64_t> g_edge16_dst_launches[PTGNN_AMD_KERNEL_EDGE16_DST_END_ - PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_];
static std::atomic<int64_t> g_beam_finish_launches[PTGNN_AMD_KERNEL_BEAM_FINISH_END_ - PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_];
static std::atomic<int64_t> g_attention16_launches[PTGNN_AMD_KERNEL_ATTENTION16_END_ - PTGNN_AMD_KERNEL_ATTENTION16_FIRST_];
static std::atomic<int64_t> g_edge16_train_launches[PTGNN_AMD_KERNEL_EDGE16_TRAIN_END_ - PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_];
static std::atomic<int64_t> *counter(int kernel_id) {
  if (kernel_id >= 0 && kernel_id < PTGNN_AMD_KERNEL_COUNT_) return &g_launches[kernel_id];
  if (kernel_id >= PTGNN_AMD_KERNEL_AGG_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_AGG_END_)
    return &g_agg_launches[kernel_id - PTGNN_AMD_KERNEL_AGG_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_CHAR_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_CHAR_END_)
    return &g_char_launches[kernel_id - PTGNN_AMD_KERNEL_CHAR_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_HEAD_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HEAD_END_)
    return &g_head_launches[kernel_id - PTGNN_AMD_KERNEL_HEAD_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_SEQ_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_SEQ_END_)
    return &g_seq_launches[kernel_id - PTGNN_AMD_KERNEL_SEQ_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_DECODE_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_DECODE_END_)
    return &g_decode_launches[kernel_id - PTGNN_AMD_KERNEL_DECODE_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_BEAM_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_BEAM_END_)
    return &g_beam_launches[kernel_id - PTGNN_AMD_KERNEL_BEAM_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_HALF_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HALF_END_)
    return &g_half_launches[kernel_id - PTGNN_AMD_KERNEL_HALF_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_END_)
    return &g_edge16_launches[kernel_id - PTGNN_AMD_KERNEL_EDGE16_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HALF_TRAIN_END_)
    return &g_half_train_launches[kernel_id - PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_DST_END_)
    return &g_edge16_dst_launches[kernel_id - PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_BEAM_FINISH_END_)
    return &g_beam_finish_launches[kernel_id - PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_ATTENTION16_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_ATTENTION16_END_)
    return &g_attention16_launches[kernel_id - PTGNN_AMD_KERNEL_ATTENTION16_FIRST_];
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_TRAIN_END_)
    return &g_edge16_train_launches[kernel_id - PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_];
  return nullptr;
}
void count_launch(int kernel_id) {
  if (std::atomic<int64_t> *c = counter(kernel_id)) c->fetch_add(1, std::memory_order_relaxed);
}

bool raise_dynamic_lds(const void *fn, size_t bytes, const char **why) {
  static std::mutex mu;
  static std::unordered_map<uint64_t, size_t> done;     // (kernel, device): the attribute is per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t key = (uint64_t)(uintptr_t)fn * 64u + (uint64_t)dev;
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find(key);
  if (it != done.end() && it->second >= bytes) return true;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (why) *why = hipGetErrorString(e);
    return false;
  }
  done[key] = bytes;
  return true;
}
}  // namespace ptgnn_amd

extern "C" int64_t ptgnn_amd_launch_count(int kernel_id) {
  std::atomic<int64_t> *c = ptgnn_amd::counter(kernel_id);
  return c ? c->load(std::memory_order_relaxed) : -1;
}

extern "C" const char *ptgnn_amd_launch_name(int kernel_id) {
  static const char *const names[PTGNN_AMD_KERNEL_COUNT_] = {
      "k_stream_linear", "k_stream_linear_ring", "k_stream_gru", "k_stream_gru_ring", "k_stream_edge",
      "k_stream_edge_shared", "k_stream_edge_v2", "k_wgrad_stream", "k_linear_tlp", "k_gru", "k_edge_linear",
      "k_edge_wgrad", "k_gather_update"};
  static const char *const agg_names[PTGNN_AMD_KERNEL_AGG_END_ - PTGNN_AMD_KERNEL_AGG_FIRST_] = {
      "k_gather_reduce", "egc_gather_combine", "egc_combine", "egc_combine_backward", "pna_aggregate",
      "pna_aggregate_backward", "attention_pool", "attention_pool_backward", "head_projection", "graph_norm",
      "graph_norm_backward", "block_attention", "block_attention_backward", "segment_scores",
      "segment_scores_backward", "embedding_bag", "embedding_bag_backward"};
  if (kernel_id >= PTGNN_AMD_KERNEL_AGG_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_AGG_END_)
    return agg_names[kernel_id - PTGNN_AMD_KERNEL_AGG_FIRST_];
  static const char *const char_names[PTGNN_AMD_KERNEL_CHAR_END_ - PTGNN_AMD_KERNEL_CHAR_FIRST_] = {
      "char_embed", "char_embed_backward", "window_max", "window_max_backward"};
  if (kernel_id >= PTGNN_AMD_KERNEL_CHAR_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_CHAR_END_)
    return char_names[kernel_id - PTGNN_AMD_KERNEL_CHAR_FIRST_];
  static const char *const head_names[PTGNN_AMD_KERNEL_HEAD_END_ - PTGNN_AMD_KERNEL_HEAD_FIRST_] = {
      "logit_loss", "logit_loss_backward", "candidate_scores", "candidate_scores_backward"};
  if (kernel_id >= PTGNN_AMD_KERNEL_HEAD_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HEAD_END_)
    return head_names[kernel_id - PTGNN_AMD_KERNEL_HEAD_FIRST_];
  static const char *const seq_names[PTGNN_AMD_KERNEL_SEQ_END_ - PTGNN_AMD_KERNEL_SEQ_FIRST_] = {
      "vocab_loss", "vocab_loss_backward", "copy_loss_finish"};
  if (kernel_id >= PTGNN_AMD_KERNEL_SEQ_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_SEQ_END_)
    return seq_names[kernel_id - PTGNN_AMD_KERNEL_SEQ_FIRST_];
  static const char *const decode_names[PTGNN_AMD_KERNEL_DECODE_END_ - PTGNN_AMD_KERNEL_DECODE_FIRST_] = {"decode_step"};
  if (kernel_id >= PTGNN_AMD_KERNEL_DECODE_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_DECODE_END_)
    return decode_names[kernel_id - PTGNN_AMD_KERNEL_DECODE_FIRST_];
  static const char *const beam_names[PTGNN_AMD_KERNEL_BEAM_END_ - PTGNN_AMD_KERNEL_BEAM_FIRST_] = {"beam_step"};
  if (kernel_id >= PTGNN_AMD_KERNEL_BEAM_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_BEAM_END_)
    return beam_names[kernel_id - PTGNN_AMD_KERNEL_BEAM_FIRST_];
  static const char *const half_names[PTGNN_AMD_KERNEL_HALF_END_ - PTGNN_AMD_KERNEL_HALF_FIRST_] = {"half_linear",
                                                                                                    "half_gru"};
  if (kernel_id >= PTGNN_AMD_KERNEL_HALF_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HALF_END_)
    return half_names[kernel_id - PTGNN_AMD_KERNEL_HALF_FIRST_];
  static const char *const edge16_names[PTGNN_AMD_KERNEL_EDGE16_END_ - PTGNN_AMD_KERNEL_EDGE16_FIRST_] = {
      "edge16", "edge16_shared"};
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_END_)
    return edge16_names[kernel_id - PTGNN_AMD_KERNEL_EDGE16_FIRST_];
  static const char *const half_train_names[PTGNN_AMD_KERNEL_HALF_TRAIN_END_ - PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_] = {
      "half_wgrad", "half_gru_train", "half_linear_add"};
  if (kernel_id >= PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_HALF_TRAIN_END_)
    return half_train_names[kernel_id - PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_];
  static const char *const edge16_dst_names[PTGNN_AMD_KERNEL_EDGE16_DST_END_ - PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_] = {
      "edge16_dst"};
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_DST_END_)
    return edge16_dst_names[kernel_id - PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_];
  static const char *const beam_finish_names[PTGNN_AMD_KERNEL_BEAM_FINISH_END_ - PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_] = {
      "beam_step_links", "beam_backtrack"};
  if (kernel_id >= PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_BEAM_FINISH_END_)
    return beam_finish_names[kernel_id - PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_];
  static const char *const attention16_names[PTGNN_AMD_KERNEL_ATTENTION16_END_ - PTGNN_AMD_KERNEL_ATTENTION16_FIRST_] = {
      "block_attention16"};
  if (kernel_id >= PTGNN_AMD_KERNEL_ATTENTION16_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_ATTENTION16_END_)
    return attention16_names[kernel_id - PTGNN_AMD_KERNEL_ATTENTION16_FIRST_];
  static const char *const edge16_train_names[PTGNN_AMD_KERNEL_EDGE16_TRAIN_END_ - PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_] = {
      "edge16_masked", "edge_wgrad16"};
  if (kernel_id >= PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_ && kernel_id < PTGNN_AMD_KERNEL_EDGE16_TRAIN_END_)
    return edge16_train_names[kernel_id - PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_];
  return kernel_id >= 0 && kernel_id < PTGNN_AMD_KERNEL_COUNT_ ? names[kernel_id] : nullptr;
}

extern "C" int ptgnn_amd_version(void) { return PTGNN_AMD_VERSION; }
extern "C" const char *ptgnn_amd_last_error(void) { return ptgnn_amd::g_err; }
