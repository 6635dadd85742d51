// The running soft-max state of a row walked ONCE -- the maximum so far and sum exp(. - maximum), so logits spanning more
// than 100 do not overflow -- in its two forms, each with a commutative merge: threads are merged by the xor butterfly
// (wave_fold: every lane ends with the same bits), then the waves in wave order (waves_in_order), both of wave_ops.h.
//
//   MaxSum  (m, s); empty is (-inf, 0).  The vocabulary loss and the decoding steps.
//   Soft    (m, s, idx): MaxSum plus where the maximum was first seen; empty is idx == kSoftNone.  The task heads.
//
// The two differ ON PURPOSE at the edges, so Soft is not written through MaxSum's push:
//   * Soft takes its FIRST element unconditionally.  A thread whose elements are all -inf holds m = -inf, s = 1 and the
//     first index: the row has an arg-max, and its lse is -inf (soft_merge counts a side with m = -inf as 0).  A leading
//     NaN becomes the maximum: a visible NaN, as torch's.
//   * MaxSum takes an element only when it compares greater.  An all -inf row stays (-inf, 0), and the callers' guard
//     `m == -inf ? 0 : logf(s)` turns that into a norm of -inf without a logf(0).
// Behind a first element of -inf and a finite second one both hold the same (m, s).
#pragma once
#include <limits.h>
#include <math.h>

#include "wave_ops.h"

namespace ptgnn_amd {

struct MaxSum {
  float m, s;
};

// commutative: combine(a, b) and combine(b, a) have the same bits
__device__ __forceinline__ MaxSum combine(const MaxSum &a, const MaxSum &b) {
  MaxSum o;
  o.m = fmaxf(a.m, b.m);
  const float sa = a.m == -INFINITY ? 0.0f : a.s * expf(a.m - o.m);
  const float sb = b.m == -INFINITY ? 0.0f : b.s * expf(b.m - o.m);
  o.s = sa + sb;
  return o;
}

__device__ __forceinline__ void push(MaxSum &a, float v) {
  if (v > a.m) {
    a.s = a.m == -INFINITY ? 0.0f : a.s * expf(a.m - v);
    a.m = v;
  }
  if (a.m != -INFINITY) a.s += expf(v - a.m);
}

// four elements at once: one rescale for their maximum, their terms added as a tree
__device__ __forceinline__ void push4(MaxSum &a, const float (&v)[4]) {
  const float gm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
  if (gm > a.m) {
    a.s = a.m == -INFINITY ? 0.0f : a.s * expf(a.m - gm);
    a.m = gm;
  }
  if (a.m != -INFINITY) a.s += (expf(v[0] - a.m) + expf(v[1] - a.m)) + (expf(v[2] - a.m) + expf(v[3] - a.m));
}

__device__ __forceinline__ MaxSum lane_xor(const MaxSum &a, int o) { return MaxSum{lane_xor(a.m, o), lane_xor(a.s, o)}; }

constexpr int kSoftNone = INT_MAX;

struct Soft {
  float m, s;
  int idx;
};

__device__ __forceinline__ Soft soft_empty() { return Soft{-INFINITY, 0.0f, kSoftNone}; }

// for elements met in ascending index order: an equal value keeps the earlier (lower) index
__device__ __forceinline__ void soft_push(Soft &a, float v, int at) {
  if (a.idx == kSoftNone || v > a.m) {
    a.s = (a.m == -INFINITY ? 0.0f : a.s * expf(a.m - v)) + 1.0f;
    a.m = v;
    a.idx = at;
  } else {
    a.s += v == -INFINITY ? 0.0f : expf(v - a.m);
  }
}

// soft_push for elements met in ANY index order (k_candidate_scores: plan order).  The one difference: an equal value
// takes over as the maximum when its index is the smaller one, where soft_push keeps the index it has.
__device__ __forceinline__ void soft_push_lowest(Soft &a, float v, int at) {
  if (a.idx == kSoftNone || v > a.m || (v == a.m && at < a.idx)) {
    a.s = (a.m == -INFINITY ? 0.0f : a.s * expf(a.m - v)) + 1.0f;
    a.m = v;
    a.idx = at;
  } else {
    a.s += v == -INFINITY ? 0.0f : expf(v - a.m);
  }
}

// commutative: soft_merge(a, b) and soft_merge(b, a) have the same bits; lowest index on equal maxima
__device__ __forceinline__ Soft soft_merge(const Soft &a, const Soft &b) {
  Soft o;
  o.m = fmaxf(a.m, b.m);
  const float sa = a.m == -INFINITY ? 0.0f : a.s * expf(a.m - o.m);
  const float sb = b.m == -INFINITY ? 0.0f : b.s * expf(b.m - o.m);
  o.s = sa + sb;
  const bool take_b = b.idx != kSoftNone && (a.idx == kSoftNone || b.m > a.m || (b.m == a.m && b.idx < a.idx));
  o.idx = take_b ? b.idx : a.idx;
  return o;
}

__device__ __forceinline__ Soft lane_xor(const Soft &a, int o) {
  return Soft{lane_xor(a.m, o), lane_xor(a.s, o), lane_xor(a.idx, o)};
}

}  // namespace ptgnn_amd
