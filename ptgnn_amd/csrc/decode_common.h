// What the decoding-step kernels share (decode_step.hip: greedy, top-1; beam_step.hip: the W best across W parents): the
// running soft-max state (MaxSum of softmax_state.h), the candidate of an arg-max, the order-preserving key of a float,
// and the radix select of the n-th largest entry of a row of raw vocabulary scores with its tie cut.  One workgroup of
// kDecThreads threads per row; thread t owns the columns t, t + kDecThreads, ... in every pass.
#pragma once
#include <math.h>

#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {

constexpr int kDecThreads = 1024;
constexpr int kDecWaves = kDecThreads / kWave;

// a candidate of an arg-max: `rank` orders equal values (decode_step: -1 the row's top-1, else the slot that starts the
// run; beam_step: the tie class of the entry)
struct Cand {
  float v;
  int rank;
  int64_t id;
};

__device__ __forceinline__ bool better(const Cand &a, const Cand &b) {
  return a.v > b.v || (a.v == b.v && a.rank < b.rank);
}

__device__ __forceinline__ Cand lane_xor(const Cand &a, int o) {
  return Cand{lane_xor(a.v, o), lane_xor(a.rank, o), lane_xor(a.id, o)};
}

// larger float <=> larger key; -0 and +0 share a key
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float score_at(const float *__restrict__ row, const float *__restrict__ bias, int c) {
  return row[c] + (bias ? bias[c] : 0.0f);
}

// not log_sum_exp2 of vocab_loss.hip, which rounds as torch.logsumexp does
__device__ __forceinline__ float log_add_exp(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (lo == -INFINITY) return hi;
  return hi + log1pf(expf(lo - hi));
}

// The n-th largest key of a row by a radix select, eight bits a pass, over the order-preserving bit pattern of the floats:
// a 256-bin histogram in LDS counted with INTEGER atomics (their result does not depend on the order of arrival); the row
// is re-read from L2.  Entries equal to the n-th value are among the n largest by lowest index first: when not all of them
// fit, a scan over the row finds the index of the last one that does.  A `__shared__` object of the workgroup.
struct RadixSelect {
  int hist[256];
  uint32_t prefix;
  int want, cut, equal;
  SegmentScan<kDecThreads> scan;

  // All kDecThreads threads call it, with 1 <= n <= vocab: column c is one of the n largest of the row
  // <=> order_key(score) > kth || (order_key(score) == kth && c <= cut_at).
  __device__ __forceinline__ void select(const float *__restrict__ row, const float *__restrict__ bias, int vocab, int n,
                                         uint32_t &kth, int &cut_at) {
    const int t = threadIdx.x;
    if (t == 0) prefix = 0, want = n, cut = INT32_MAX;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0;
      __syncthreads();
      const uint32_t pre = prefix;
      for (int c = t; c < vocab; c += kDecThreads) {
        const uint32_t key = order_key(score_at(row, bias, c));
        if (shift == 24 || (key >> (shift + 8)) == (pre >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      // bins from the largest down: thread t < 256 has bin 255 - t; the bin where the running count reaches `want`
      const int count = t < 256 ? hist[255 - t] : 0;
      const int need = want;
      scan.begin();
      const int before = scan.step(count);
      if (t < 256 && before < need && before + count >= need) {
        prefix = pre | ((uint32_t)(255 - t) << shift);
        want = need - before;
        equal = count;                                       // after the last pass: the entries with the n-th key
      }
      __syncthreads();
    }
    kth = prefix;
    const int need = want;                                   // how many of the entries with key == kth are in the n
    if (need < equal) {                                      // workgroup-uniform: an exact tie at the n-th place
      scan.begin();
      for (int base = 0; base < vocab; base += kDecThreads) {
        const int c = base + t;
        const int hit = c < vocab && order_key(score_at(row, bias, c)) == kth ? 1 : 0;
        const int before = scan.step(hit);
        if (hit && before == need - 1) cut = c;
      }
      __syncthreads();
    }
    cut_at = cut;
    __syncthreads();                                         // the object may be used again
  }
};

}  // namespace ptgnn_amd
