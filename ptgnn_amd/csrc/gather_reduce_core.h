// Shared core of the CSR aggregation kernels: the lane-group row walk (RowOp), the hub-chunk and long-row launches
// and their launch plumbing.  Included by gather_reduce.hip (ptgnn_amd_gather_reduce_*) and egc_combine.hip (the
// aggregation with the EGC head / basis combination as its row finish), so both walk a plan the same way.
//
// Contract + reference lines: include/ptgnn_amd.h (ptgnn_amd_gather_reduce_f32).
//
// Mapping (HBM/L2-bound, no MFMA on purpose):
//   * one destination row per group of LPR lanes, LPR = msg_dim/4 rounded to {16,32,64}; each lane
//     owns CH float4 column chunks => a 64-lane wave reads 1 KiB of message rows per
//     wave-instruction (16 B/lane, the coalescing sweet spot), 64/LPR rows per wave;
//   * the in-edges of a row are contiguous in `col` (CSR) and folded IN ORDER, so fp32 sums are
//     deterministic and follow the reference's message order; no atomics;
//   * the edge loop runs in groups of 8 slots (4 with a destination term) with all row loads of a group
//     issued before the first use and the next group's `col` entries fetched behind them: 8 KiB per wave
//     in flight, one round trip per group;
//   * consecutive row tiles run on the same XCD (xcd_swizzle) so one graph of a disjoint-union
//     batch keeps its node states in a single 4 MiB L2;
//   * HUB rows (in-degree > hub_threshold, power-law graphs): one lane group folding 10^5..10^6
//     edges serially would set the kernel's duration, so such rows are skipped by the main kernel
//     and split over 1024-slot chunks: the plan lists every (chunk, hub row) pair once per
//     minibatch (ptgnn_amd_csr_build), and ONE small extra launch walks that list: a workgroup
//     reduces its chunk of the hub with all its lane groups (slot-interleaved, combined in a fixed
//     order), publishes the partial, and the LAST chunk of a hub to arrive (one ticket counter per
//     hub, agent-scope release/acquire) folds the partials in chunk order and applies the row
//     epilogue -- deterministic values, no float atomics.  The fold ORDER of a hub row differs from
//     the reference's serial order (fp32 rounding only; max/min and their arg stay exact).  A plan
//     without hubs costs one ~2 us launch whose workgroups read a zero count and exit.
// Algorithmic bytes per edge: 4*M (message row) + 4 (col) ; per node: 4*M (out) [+ 4*M dst term].
#pragma once
#include <float.h>
#include <stdlib.h>

#include <type_traits>

#include <mutex>

#include "dense_common.h"   // f32x16, kcol(), act_apply(): the fused node update below multiplies like the GEMM kernels
#include "wave_ops.h"       // group_sum: the LayerNorm of the node update

namespace ptgnn_amd {

// ------------------------------------------------------------------------------------------------
// launch plumbing
// ------------------------------------------------------------------------------------------------
// The hub launch is independent of the main launch (disjoint rows), both are bandwidth-bound, and each has a tail
// (the main kernel: its last long rows, one wave each; the hub kernel: the last chunks of the largest hub) -- so the
// hub kernel runs on a SIDE stream of the library, forked from and joined back into the caller's stream with events
// (the fork-join pattern that is also legal under stream capture): the two overlap instead of queueing.
// PTGNN_AMD_HUB_STREAM=0 keeps both on the caller's stream (A/B).
// One set of side streams + events per (device, CALLER STREAM): two caller streams on one device -- or two host threads --
// never share a fork / join event (a shared set let one caller's join wait on the other's record and read its output
// before its hub rows were written; ADVICE / VERDICT r03).  `mu` serialises the fork .. join enqueue sequence of callers
// that do use the same stream from two threads; the pool is looked up under `g_side_mu`.  Entries are created on first
// use OUTSIDE a stream capture (creating streams / events is not capturable: a first use inside a capture stays on one
// stream) and live for the process; beyond kSidePool distinct caller streams the launches stay on the caller's stream.
struct SideStream {
  int dev = -1;
  hipStream_t owner = nullptr;     // the caller's stream this set belongs to
  hipStream_t stream = nullptr;    // hub chunks
  hipStream_t stream2 = nullptr;   // long rows
  hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
  std::mutex mu;
};

// the caller stream's set (gather_reduce.hip), created if `may_create` (not capturing) and there is room; else nullptr
SideStream *side_stream(hipStream_t caller, bool may_create);

namespace {

constexpr int kHubChunk = 1024;  // CSR slots per hub chunk; hub_threshold must be >= 2 * kHubChunk
constexpr int kLongRow = 256;    // rows beyond this many in-edges fold in their own launch (k_long_rows)

struct Args {
  const float *ysrc;
  const float *ydst;
  int64_t ld_y;
  int64_t ld_yd;
  const int32_t *rowptr;
  const int32_t *col;
  const int32_t *hdr;        // nullable [num rows, 8]: col[rowptr[r] + k] clamped to the row's last slot (row_hdr of the ABI)
  int32_t type_bits;
  int64_t num_nodes;         // one past the last row of this launch
  int64_t row_begin;         // first row of this launch (0 unless a row range was asked for); pointers stay absolute
  int32_t msg_dim;
  const float *ln_gamma;
  const float *ln_beta;
  float ln_eps;
  float *out;
  int64_t ld_out;
  int32_t *argout;
  int64_t num_tiles;
  int32_t epi;
  const int32_t *mask_arg;   // MASKED: [num source rows of this launch, M] winning forward slot
  const int32_t *mask_slot;  // MASKED: [E] forward slot of each slot of THIS plan
  int32_t hub_threshold;     // rows with more in-edges are left to the hub kernels (0 = no hub path)
  int32_t long_threshold;    // rows with more in-edges (up to hub_threshold) are left to k_long_rows (0 = none)
  int32_t hub_blocks;        // leading workgroups of the main launch that walk the hub list (0: a launch of its own does)
  float *hub_part;           // [2 * num_chunks, M] chunk partials
  int32_t *hub_arg;          // [2 * num_chunks, M] (argout only)
  int32_t *hub_tickets;      // [num_chunks * col_blocks] arrival counters, zero between launches
  const int32_t *hub_entries;  // plan: (chunk, row) pairs
  const int32_t *hub_count;    // plan: number of pairs
  int64_t num_edges;
  // COMB (egc_combine.hip): the finished row [K, B, Dh] leaves as out_c[v, k*Dh + d] = sum_b coef[v, k*B + b] * row[k, b, d]
  const float *coef;         // [rows, K*B], leading dimension ld_coef
  int64_t ld_coef;
  float *comb_out;           // [rows, K*Dh], leading dimension ld_comb
  int64_t ld_comb;
  int32_t comb_heads, comb_bases, comb_dh;
  int32_t comb_vec4;         // Dh % 4 == 0 and 16-byte output rows: float4 stores
};

// Per-lane-group state and the steps every kernel composes: fold a slot range, fold another partial,
// finish + store the row.  VEC = 4: float4 path (msg_dim % 4 == 0, 16-B aligned rows); VEC = 1:
// generic.  MASKED (sum only): the gathered row is an output gradient that only flows where the
// forward max/min picked this very edge:  value = (mask_arg[src, c] == mask_slot[i]) ? row[c] : 0.
// COMB: the row finish is the EGC head / basis combination (combine_store) instead of a plain store.
template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool COMB = false>
struct RowOp {
  const Args &a;
  const int g, cbase, M;
  const int32_t tmask;
  float acc[CH][VEC];
  int arg[CH][VEC];

  static constexpr float kInit =
      REDUCE == PTGNN_AMD_MAX ? -FLT_MAX : (REDUCE == PTGNN_AMD_MIN ? FLT_MAX : 0.f);

  __device__ __forceinline__ RowOp(const Args &a_, int g_, int cbase_)
      : a(a_), g(g_), cbase(cbase_), M(a_.msg_dim), tmask((1 << a_.type_bits) - 1) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) { acc[c][v] = kInit; arg[c][v] = -1; }
  }

  __device__ __forceinline__ void load_row(const float *base, float (&dst)[CH][VEC]) const {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int colx = cbase + (g + c * LPR) * VEC;
      if constexpr (VEC == 4) {
        if (colx < M) {
          const float4 t = *reinterpret_cast<const float4 *>(base + colx);
          dst[c][0] = t.x; dst[c][1] = t.y; dst[c][2] = t.z; dst[c][3] = t.w;
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) dst[c][v] = 0.f;
        }
      } else {
        dst[c][0] = colx < M ? base[colx] : 0.f;
      }
    }
  }

  __device__ __forceinline__ void apply_mask(float (&m)[CH][VEC], int64_t srow, int i) const {
    if constexpr (MASKED) {
      const int want = a.mask_slot[i];
      const int32_t *ar = a.mask_arg + srow * (int64_t)M;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int colx = cbase + (g + c * LPR) * VEC;
        if constexpr (VEC == 4) {
          if (colx < M) {
            const int4 w = *reinterpret_cast<const int4 *>(ar + colx);
            m[c][0] = w.x == want ? m[c][0] : 0.f; m[c][1] = w.y == want ? m[c][1] : 0.f;
            m[c][2] = w.z == want ? m[c][2] : 0.f; m[c][3] = w.w == want ? m[c][3] : 0.f;
          }
        } else {
          if (colx < M) m[c][0] = ar[colx] == want ? m[c][0] : 0.f;
        }
      }
    }
  }

  // fold one candidate (value, slot); on max/min ties the earlier slot stays (torch_scatter's arg)
  __device__ __forceinline__ void fold(const float (&m)[CH][VEC], int slot) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (REDUCE == PTGNN_AMD_MAX) {
          if (m[c][v] > acc[c][v]) { acc[c][v] = m[c][v]; if (HAS_ARG) arg[c][v] = slot; }
        } else if (REDUCE == PTGNN_AMD_MIN) {
          if (m[c][v] < acc[c][v]) { acc[c][v] = m[c][v]; if (HAS_ARG) arg[c][v] = slot; }
        } else {
          acc[c][v] += m[c][v];
        }
      }
  }

  // fold a partial whose slots are not ordered w.r.t. ours (interleaved groups): ties -> lower slot
  __device__ __forceinline__ void fold_partial(const float (&m)[CH][VEC], const int (&ma)[CH][VEC]) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN) {
          const bool better = REDUCE == PTGNN_AMD_MAX ? m[c][v] > acc[c][v] : m[c][v] < acc[c][v];
          bool take = better;
          if (HAS_ARG)
            take = better || (m[c][v] == acc[c][v] && ma[c][v] >= 0 && (arg[c][v] < 0 || ma[c][v] < arg[c][v]));
          if (take) { acc[c][v] = m[c][v]; if (HAS_ARG) arg[c][v] = ma[c][v]; }
        } else {
          acc[c][v] += m[c][v];
        }
      }
  }

  // slots beg, beg+stride, ... < end of destination row `row`
  __device__ __forceinline__ void reduce(int64_t row, int beg, int end, int stride) {
    const float *dst_base = HAS_DST ? a.ydst + row * a.ld_yd : nullptr;
    constexpr int U = 4;
    int i = beg;
    for (; i + (U - 1) * stride < end; i += U * stride) {
      int32_t pk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) pk[u] = a.col[i + u * stride];
      float m[U][CH][VEC];
      float d[U][CH][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t s = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        load_row(a.ysrc + s * a.ld_y + (int64_t)t * M, m[u]);
        apply_mask(m[u], s, i + u * stride);
        if (HAS_DST) load_row(dst_base + (int64_t)t * M, d[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (HAS_DST) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] += d[u][c][v];
        }
        fold(m[u], i + u * stride);
      }
    }
    if (i < end) {
      // tail of 1 .. U-1 slots as ONE more group: indices clamped to the last slot (unconditional loads,
      // all in flight together) instead of a serial col -> row -> fold chain per slot.  A duplicate of
      // the last slot is idempotent for max/min (strict compare) and is zeroed for the sums.
      const int last = i + ((end - 1 - i) / stride) * stride;
      constexpr int TU = U - 1;   // the tail holds at most U - 1 slots
      int32_t pk[TU];
      int idx[TU];
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        idx[u] = i + u * stride < end ? i + u * stride : last;
        pk[u] = a.col[idx[u]];
      }
      float m[TU][CH][VEC];
      float d[TU][CH][VEC];
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int64_t s = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        load_row(a.ysrc + s * a.ld_y + (int64_t)t * M, m[u]);
        apply_mask(m[u], s, idx[u]);
        if (HAS_DST) load_row(dst_base + (int64_t)t * M, d[u]);
      }
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const bool valid = i + u * stride < end;
        if (HAS_DST) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] += d[u][c][v];
        }
        if (REDUCE != PTGNN_AMD_MAX && REDUCE != PTGNN_AMD_MIN) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] = valid ? m[u][c][v] : 0.f;
        }
        fold(m[u], idx[u]);
      }
    }
  }

  // The same fold as reduce() in groups of U slots, every group ONE round trip: the group's U `col` entries
  // were fetched while the previous group's rows were in flight (the first group's together, up front), and a
  // short row or a tail is a clamped group (duplicates of the row's last slot: idempotent for max / min, zeroed
  // for the sums) instead of a second, smaller round trip.  Slots fold in CSR order: bit-identical to reduce()
  // (checked on the GPU over widths / reduces / args / epilogues / hub and tail cases,
  // scripts/experiments/gr_walk_ab.py).  U = 8 keeps the kernel at 63-70 VGPRs (7-8 waves per SIMD) with twice
  // the bytes in flight per wave: cfg3 97 -> 89 us, cfg5 shard 4.20 -> 3.39 ms (a 4000-edge row was ~1000 serial
  // col -> row round trips; now ~500 single ones).
  // DST_ONCE (one edge type: the destination term is the same row for every slot): it is loaded once per row
  // instead of once per slot; every slot still folds (message + destination term), same bits.
  template <int U, bool DST_ONCE = false>
  __device__ __forceinline__ void reduce_pf(int64_t row, int beg, int end, int stride) {
    if (beg >= end) return;
    const float *dst_base = HAS_DST ? a.ydst + row * a.ld_yd : nullptr;
    const int last = beg + ((end - 1 - beg) / stride) * stride;
    float d1[CH][VEC];
    if constexpr (HAS_DST && DST_ONCE) load_row(dst_base, d1);
    int32_t pk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = beg + u * stride;
      pk[u] = a.col[idx < last ? idx : last];
    }
    for (int i = beg; i < end; i += U * stride) {
      float m[U][CH][VEC];
      float d[(HAS_DST && !DST_ONCE) ? U : 1][CH][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t s = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        const int idx = i + u * stride;
        load_row(a.ysrc + s * a.ld_y + (int64_t)t * M, m[u]);
        apply_mask(m[u], s, idx < last ? idx : last);
        if constexpr (HAS_DST && !DST_ONCE) load_row(dst_base + (int64_t)t * M, d[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {   // the next group's col entries ride behind this group's rows
        const int idx = i + (U + u) * stride;
        pk[u] = a.col[idx < last ? idx : last];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = i + u * stride;
        const bool valid = idx < end;
        if constexpr (HAS_DST) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] += DST_ONCE ? d1[c][v] : d[DST_ONCE ? 0 : u][c][v];
        }
        if (REDUCE != PTGNN_AMD_MAX && REDUCE != PTGNN_AMD_MIN) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] = valid ? m[u][c][v] : 0.f;
        }
        fold(m[u], valid ? idx : last);
      }
    }
  }

  // The header-first walk of the main kernel: the fold of reduce_pf<U>(row, beg, end, 1) with the first group's U
  // entries already in registers -- `first`, the row's header record (Args::hdr), requested together with the rowptr
  // pair: the same clamped entries reduce_pf fetches once `beg` is known, one dependent round trip earlier.  That group
  // is folded on its own, ahead of the loop (one loop body fed from the header on entry and from `col` on the back
  // edge makes the compiler wait for every row load before it issues the next).  The further groups of a longer row
  // (8 % of the rows of a code graph) fetch their entries at the top of the group, which is also where the compiler
  // puts reduce_pf's prefetch: no entries carried across the fold keeps this walk inside the plain one's registers.
  // Slots past the row's end are not loaded here (reduce_pf loads a duplicate of the last slot): the lanes of a slot
  // load under the mask they already have for the column bound, and the slot folds the value that changes nothing --
  // 0 into a sum, as there; the accumulator's initial value into a max / min, which a strict compare never takes,
  // exactly like a duplicate of a value that is already folded.  Same slots, same order: same bits, and a row of 3
  // in-edges has 3 row loads in flight, not 8.
  template <int U>
  __device__ __forceinline__ void reduce_hdr(int beg, int end, const int32_t (&first)[U]) {
    static_assert(VEC == 4 && !MASKED && !HAS_ARG && !HAS_DST, "the header walk serves plain float4 rows");
    if (beg >= end) return;
    fold_group<U>(first, beg, end);
    for (int i = beg + U; i < end; i += U) {
      int32_t pk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) pk[u] = a.col[i + u < end ? i + u : end - 1];
      fold_group<U>(pk, i, end);
    }
  }

  // reduce_hdr: the slots i, i + 1, ... < end of a group of U whose col entries are `pk` (clamped, so every address is
  // a valid one): all row loads issued before any is used, then folded in slot order
  template <int U>
  __device__ __forceinline__ void fold_group(const int32_t (&pk)[U], int i, int end) {
    constexpr bool kMinMax = REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN;
    float m[U][CH][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t s = pk[u] >> a.type_bits;
      const int t = pk[u] & tmask;
      const float *base = a.ysrc + s * a.ld_y + (int64_t)t * M;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int colx = cbase + (g + c * LPR) * VEC;
        if (colx < M && i + u < end) {
          const float4 v = *reinterpret_cast<const float4 *>(base + colx);
          m[u][c][0] = v.x; m[u][c][1] = v.y; m[u][c][2] = v.z; m[u][c][3] = v.w;
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) m[u][c][v] = 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = i + u < end;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) m[u][c][v] = valid ? m[u][c][v] : (kMinMax ? kInit : 0.f);
      fold(m[u], i + u);
    }
  }

  __device__ __forceinline__ void store(float *orow, int32_t *arow) const {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int colx = cbase + (g + c * LPR) * VEC;
      if (colx >= M) continue;
      if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(orow + colx) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        if (HAS_ARG) *reinterpret_cast<int4 *>(arow + colx) = make_int4(arg[c][0], arg[c][1], arg[c][2], arg[c][3]);
      } else {
        orow[colx] = acc[c][0];
        if (HAS_ARG) arow[colx] = arg[c][0];
      }
    }
  }

  // mean / empty-segment rule / row epilogue / store
  __device__ __forceinline__ void finish_and_store(int64_t row, int deg) {
    finish(deg);
    if constexpr (COMB) combine_store(row);
    else store(a.out + row * a.ld_out, HAS_ARG ? a.argout + row * (int64_t)M : nullptr);
  }

  // EGC combine of the finished row (whole row in this lane group: one column block, cbase == 0).  The row is staged in
  // LDS -- one slot of LPR*VEC*CH floats per lane group, indexed by threadIdx.x / LPR, which is unique for the row's lane
  // group in every kernel that finishes rows (main, hub finisher, long rows) -- and each lane then produces output
  // columns j = k*Dh + d as sum_b coef[k*B + b] * row[k*B*Dh + b*Dh + d], b in order.  The aggregate itself (and the
  // arg of max / min) is stored only when the caller asked for it (a.out / a.argout non-null: training).
  __device__ __forceinline__ void combine_store(int64_t row) {
    __shared__ __attribute__((aligned(16))) float stage[256 * VEC * CH];
    if (a.out != nullptr) store(a.out + row * a.ld_out, HAS_ARG ? a.argout + row * (int64_t)M : nullptr);
    float *srow = stage + (threadIdx.x / LPR) * (LPR * VEC * CH);
    wave_sync();   // readers of this slot's previous row (hub / long-row loops) are done
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int colx = (g + c * LPR) * VEC;
      if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(srow + colx) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
      } else {
        srow[colx] = acc[c][0];
      }
    }
    wave_sync();
    const int K = a.comb_heads, B = a.comb_bases, Dh = a.comb_dh, D = K * Dh;
    const float *cw = a.coef + row * a.ld_coef;
    float *orow = a.comb_out + row * a.ld_comb;
    if (a.comb_vec4) {
      for (int q = g; q < D / 4; q += LPR) {
        const int j = 4 * q, k = j / Dh, d = j - k * Dh;
        const float *base = srow + k * B * Dh + d;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < B; ++b) {
          const float w = cw[k * B + b];
          const float4 t = *reinterpret_cast<const float4 *>(base + b * Dh);
          s.x += w * t.x; s.y += w * t.y; s.z += w * t.z; s.w += w * t.w;
        }
        *reinterpret_cast<float4 *>(orow + j) = s;
      }
    } else {
      for (int j = g; j < D; j += LPR) {
        const int k = j / Dh, d = j - k * Dh;
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += cw[k * B + b] * srow[k * B * Dh + b * Dh + d];
        orow[j] = s;
      }
    }
  }

  // the lane group lives inside one wave: a wave-level barrier orders its LDS writes and reads (other lane groups of the
  // wave may have left the kernel)
  static __device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }

  // mean / empty-segment rule / row epilogue, left in `acc`
  __device__ __forceinline__ void finish(int deg) {
    const int EPI = a.epi;  // wave-uniform
    if (REDUCE == PTGNN_AMD_MEAN) {
      const float cnt = (float)(deg < 1 ? 1 : deg);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[c][v] = acc[c][v] / cnt;
    }
    if ((REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN) && deg == 0) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[c][v] = 0.f;  // torch_scatter: empty segment -> 0
    }
    if (EPI & PTGNN_AMD_EPI_GELU) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[c][v] = gelu_erf(acc[c][v]);
    }
    if (EPI & PTGNN_AMD_EPI_LAYERNORM) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) s += ((g + c * LPR) * VEC + v < M) ? acc[c][v] : 0.f;
      const float mean = group_sum<LPR>(s) / (float)M;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float dlt = acc[c][v] - mean;
          q += ((g + c * LPR) * VEC + v < M) ? dlt * dlt : 0.f;
        }
      const float rstd = 1.0f / sqrtf(group_sum<LPR>(q) / (float)M + a.ln_eps);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int colx = (g + c * LPR) * VEC + v;
          if (colx < M) acc[c][v] = (acc[c][v] - mean) * rstd * a.ln_gamma[colx] + a.ln_beta[colx];
        }
    }
  }

  __device__ __forceinline__ void load_partial(const float *prow, const int32_t *parow,
                                               float (&m)[CH][VEC], int (&ma)[CH][VEC]) const {
    load_row(prow, m);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int colx = cbase + (g + c * LPR) * VEC;
#pragma unroll
      for (int v = 0; v < VEC; ++v) ma[c][v] = (HAS_ARG && colx + v < M) ? parow[colx + v] : -1;
    }
  }
};

// ------------------------------------------------------------------------------------------------
// hub kernel: workgroups walk the plan's (chunk, hub row) list
// ------------------------------------------------------------------------------------------------
#ifndef PTGNN_HUB_FUSED_BLOCKS
#define PTGNN_HUB_FUSED_BLOCKS 32      // A/B knob (scripts/build_variant.sh): 0 = the hub launch of its own everywhere
#endif
template <int CH, bool HAS_DST, bool HAS_ARG, bool MASKED>
constexpr bool hub_fuses() { return PTGNN_HUB_FUSED_BLOCKS > 0 && CH == 1 && !HAS_DST && !HAS_ARG && !MASKED; }
// The destination-term variants (MLP-MP table form) can walk the hub list inside the main launch too, but pay for it with
// registers: measured in round 6 (profiles/r06_notes.md 6), BASELINE config 2 (1.1 M edges, 144 us launch) gets 1.5 % SLOWER,
// the 80-150 k-edge minibatches of config 1 (19 us launches, five per forward) 5.8 % faster.  So it is a second instantiation,
// taken below this many edges.
constexpr int64_t kFuseDstMaxEdges = (int64_t)1 << 19;
template <int CH, bool HAS_DST, bool HAS_ARG, bool MASKED>
constexpr bool hub_fuses_small() { return PTGNN_HUB_FUSED_BLOCKS > 0 && CH == 1 && HAS_DST && !HAS_ARG && !MASKED; }

template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool FUSED = false,
          bool COMB = false>
__device__ __forceinline__ void hub_chunks_body(const Args &a, int first, int stride) {
  using Op = RowOp<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, COMB>;
  constexpr int G = 256 / LPR;          // lane groups per workgroup
  constexpr int W = LPR * VEC * CH;     // columns per column block
  __shared__ float pv[G * W];
  __shared__ int pa[HAS_ARG ? G * W : 1];

  const int count = *a.hub_count;
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int cbase = blockIdx.y * W;
  const int64_t num_chunks = (a.num_edges + kHubChunk - 1) / kHubChunk;
#pragma unroll 1
  for (int e = first; e < count; e += stride) {
    const int64_t chunk = a.hub_entries[2 * e];
    const int64_t row = a.hub_entries[2 * e + 1];
    if (row < a.row_begin || row >= a.num_nodes) continue;   // a row-range launch: the hub belongs to another piece
    const int64_t cbeg = chunk * kHubChunk;
    const int64_t cend = (cbeg + kHubChunk < a.num_edges) ? cbeg + kHubChunk : a.num_edges;
    const int rbeg = a.rowptr[row], rend = a.rowptr[row + 1];
    const int sbeg = (int)(rbeg > cbeg ? rbeg : cbeg), send = (int)(rend < cend ? rend : cend);
    // partial slot of this (chunk, row): 0 if the hub owns the chunk's first slot, else 1
    const int which = rbeg <= cbeg ? 0 : 1;
    Op op(a, g, cbase);
    // the chunk's slots are interleaved over the lane groups (stride G); same prefetched groups of 8 as the main kernel.
    // max / min without an arg have nothing to break a tie of -0.0 and +0.0 with when the partials combine: there each
    // lane group folds a contiguous run of the chunk instead, so the fixed combine order below is slot order and the
    // earliest slot's zero stays, as in the serial fold (torch_scatter)
    constexpr int UP = (VEC == 4 && !MASKED && !HAS_DST && CH == 1) ? (FUSED ? 4 : 8) : 0;
    constexpr bool kRuns = (REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN) && !HAS_ARG;
    const int per = kRuns ? (send - sbeg + G - 1) / G : 0;
    const int rb = kRuns ? sbeg + grp * per : sbeg + grp;
    const int re = kRuns ? (rb + per < send ? rb + per : send) : send;
    if constexpr (UP == 0) op.reduce(row, rb, re, kRuns ? 1 : G);
    else op.template reduce_pf<UP>(row, rb, re, kRuns ? 1 : G);
    __syncthreads();  // the previous entry's readers are done with the staging arrays
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        pv[grp * W + (g + c * LPR) * VEC + v] = op.acc[c][v];
        if (HAS_ARG) pa[grp * W + (g + c * LPR) * VEC + v] = op.arg[c][v];
      }
    __syncthreads();
    if (grp != 0) continue;           // group 0 (part of wave 0) finishes the entry
    for (int q = 1; q < G; ++q) {     // fixed combine order => deterministic
      float m[CH][VEC];
      int ma[CH][VEC];
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          m[c][v] = pv[q * W + (g + c * LPR) * VEC + v];
          ma[c][v] = HAS_ARG ? pa[q * W + (g + c * LPR) * VEC + v] : -1;
        }
      op.fold_partial(m, ma);
    }
    const int64_t c_first = rbeg / kHubChunk, c_last = (rend - 1) / kHubChunk;
    op.store(a.hub_part + (2 * chunk + which) * (int64_t)a.msg_dim,
             HAS_ARG ? a.hub_arg + (2 * chunk + which) * (int64_t)a.msg_dim : nullptr);
    // publish: every storing lane releases at agent scope, then ONE lane takes a ticket
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int32_t *ticket = a.hub_tickets + (int64_t)blockIdx.y * num_chunks + c_first;
    int arrived = 0;
    if (g == 0) arrived = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    arrived = __shfl(arrived, 0, LPR);
    if (arrived != (int)(c_last - c_first)) continue;   // not the last chunk of this hub
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop stale L1 lines before reading partials
    if (g == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // self-clean
    Op fin(a, g, cbase);
    // chunk partials fold in chunk order, fetched FB at a time (a 150 k-edge hub has ~150 of them: loaded one by
    // one, this fold was most of the hub launch on the cfg5 shard)
    // (FUSED: inside the main kernel the body must fit ITS register budget -- minibatch-sized plans, short hub lists)
    constexpr int FB = FUSED ? 2 : ((HAS_ARG || CH > 1) ? 4 : 8);
    for (int64_t c0 = c_first; c0 <= c_last; c0 += FB) {
      float m[FB][CH][VEC];
      int ma[FB][CH][VEC];
#pragma unroll
      for (int u = 0; u < FB; ++u) {
        const int64_t c = c0 + u <= c_last ? c0 + u : c_last;
        const int w2 = (c > c_first || rbeg == (int)(c_first * kHubChunk)) ? 0 : 1;
        fin.load_partial(a.hub_part + (2 * c + w2) * (int64_t)a.msg_dim,
                         HAS_ARG ? a.hub_arg + (2 * c + w2) * (int64_t)a.msg_dim : nullptr, m[u], ma[u]);
      }
#pragma unroll
      for (int u = 0; u < FB; ++u)
        if (c0 + u <= c_last) fin.fold_partial(m[u], ma[u]);
    }
    fin.finish_and_store(row, rend - rbeg);
  }
}

template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool COMB = false>
__global__ __launch_bounds__(256) void k_hub_chunks(Args a) {
  hub_chunks_body<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, false, COMB>(a, (int)blockIdx.x, (int)gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// main kernel: one row per lane group
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool DST1 = false,
          bool HUBF = hub_fuses<CH, HAS_DST, HAS_ARG, MASKED>(), bool COMB = false, bool HDR = false>
__global__ __launch_bounds__(256) void k_gather_reduce(Args a) {
  constexpr int ROWS_PER_BLOCK = 256 / LPR;
  // the first `hub_blocks` workgroups (a multiple of 8: the XCD mapping of the row tiles is unchanged) walk the plan's
  // hub list instead of row tiles -- on a minibatch-sized plan the list is almost always empty and they leave at once,
  // where a hub launch of its own behind this one cost ~4.6 us of dependent launch latency per aggregation
  // (only the variants whose register budget -- 8 / 7 waves per SIMD -- the hub body fits: plain rows, one column chunk)
  if constexpr (HUBF) {
    if ((int)blockIdx.x < a.hub_blocks) {
      hub_chunks_body<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, true, COMB>(a, (int)blockIdx.x, a.hub_blocks);
      return;
    }
  }
  const int64_t tile = xcd_swizzle(blockIdx.x - a.hub_blocks, gridDim.x - a.hub_blocks);
  if (tile >= a.num_tiles) return;
  const int64_t row = a.row_begin + tile * ROWS_PER_BLOCK + threadIdx.x / LPR;
  if (row >= a.num_nodes) return;  // whole lane-group exits together (no cross-group shuffles)
  // plain rows fold in prefetched groups of 8 (4 when a lane owns two column chunks); so do rows with a
  // destination term when there is ONE edge type (DST1: the term is loaded once per row).  A per-slot destination
  // term (several edge types) stays on groups of 4: its second row set per slot would cost the occupancy the
  // wider group buys.
  constexpr int UP = (VEC == 4 && !MASKED && (!HAS_DST || DST1)) ? (CH == 1 ? 8 : 4) : 0;
  // HDR, the header-first walk (groups of 8 only; launch_main picks it when the caller gave row headers): the row's
  // header record holds the first group's eight col entries at an address that depends on `row` alone, so it is
  // requested TOGETHER with the rowptr pair and the first payload group starts one round trip earlier
  // (rowptr + header -> rows, instead of rowptr -> col -> rows).
  static_assert(!HDR || UP == 8, "row headers serve the walks in groups of 8");
  int32_t pk[HDR ? 8 : 1];
  int beg, end;
  if constexpr (HDR) {
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 *rec = reinterpret_cast<const i32x4 *>(a.hdr + row * 8);
    i32x4 h0 = rec[0], h1 = rec[1];
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
    // No instruction: the record and the rowptr pair are all "used" here, ahead of the branches on the row's degree.
    // Without it the compiler sinks the record's loads to their first use, behind the wait for the rowptr pair --
    // the dependent round trip the record is there to remove.
    asm volatile("" : "+v"(h0), "+v"(h1), "+v"(beg), "+v"(end));
    pk[0] = h0.x; pk[1] = h0.y; pk[2] = h0.z; pk[3] = h0.w;
    pk[4] = h1.x; pk[5] = h1.y; pk[6] = h1.z; pk[7] = h1.w;
  } else {
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
  }
  if (a.hub_threshold > 0 && end - beg > a.hub_threshold) return;  // hub: the chunk kernel owns it
  if (a.long_threshold > 0 && end - beg > a.long_threshold) return;  // long row: k_long_rows owns it
  // column block (only > 0 when msg_dim exceeds LPR*VEC*CH; epilogues are then disabled by host)
  RowOp<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, COMB> op(a, threadIdx.x % LPR,
                                                               blockIdx.y * (LPR * VEC * CH));
  if constexpr (UP == 0) op.reduce(row, beg, end, 1);
  else if constexpr (HDR) op.template reduce_hdr<8>(beg, end, pk);
  else op.template reduce_pf<UP, HAS_DST && DST1>(row, beg, end, 1);
  op.finish_and_store(row, end - beg);
}

// ------------------------------------------------------------------------------------------------
// long rows (long_threshold < in-degree <= hub_threshold), on the side stream next to the main launch
// ------------------------------------------------------------------------------------------------
// A row of 2048 in-edges folded by one lane group of the main kernel is 256 dependent round trips (~0.5 ms on a
// 2.6 ms launch): wherever it starts, the launch cannot end before it does, and on a power-law graph some start
// late.  These rows fold in the SAME slot order (bit-identical sums) but 16 slots per round trip, in a launch of
// their own that starts together with the main one.  A wave scans 64 consecutive rowptr entries per load and visits
// the long rows among them one at a time on its first LPR lanes.
template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool COMB = false>
__global__ __launch_bounds__(256) void k_long_rows(Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
  for (int64_t base = a.row_begin + wave * 64; base < a.num_nodes; base += nwaves * 64) {
    const int64_t r = base + lane;
    int beg = 0, deg = 0;
    if (r < a.num_nodes) {
      beg = a.rowptr[r];
      deg = a.rowptr[r + 1] - beg;
    }
    unsigned long long todo = __ballot(deg > a.long_threshold && deg <= a.hub_threshold);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int rbeg = __shfl(beg, b, 64), rdeg = __shfl(deg, b, 64);
      if (lane < LPR) {
        RowOp<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, false, COMB> op(a, lane, blockIdx.y * (LPR * VEC * CH));
        op.template reduce_pf<16, HAS_DST>(base + b, rbeg, rbeg + rdeg, 1);   // HAS_DST: one edge type (host checks)
        op.finish_and_store(base + b, rdeg);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// launch plumbing
// ------------------------------------------------------------------------------------------------
// Which main-kernel variants have a header-first instantiation: plain float4 rows in one column chunk, walked in groups
// of 8, without mask, destination term or arg output.  Their header form keeps or gains waves per SIMD against the plain
// one (the compiler's kernel-resource-usage remarks, tabulated in profiles/row_headers_notes.md).  Every other variant
// ignores Args::hdr.  Left on the plain walk because a header form cost them waves when it was built: max / min with
// an arg output (63 -> 74 VGPRs, 8 -> 6 waves per SIMD) and every variant with a destination term (62-79 -> 236-238
// VGPRs, 2 waves).
template <int VEC, int CH, bool HAS_DST, bool HAS_ARG, bool MASKED, bool COMB>
constexpr bool hdr_walk() {
  return VEC == 4 && CH == 1 && !MASKED && !COMB && !HAS_ARG && !HAS_DST;
}

template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool DST1, bool HUBF, bool COMB>
void launch_main(const Args &a, dim3 grid, hipStream_t stream) {
  if constexpr (hdr_walk<VEC, CH, HAS_DST, HAS_ARG, MASKED, COMB>()) {
    if (a.hdr != nullptr) {
      k_gather_reduce<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, DST1, HUBF, COMB, true><<<grid, 256, 0, stream>>>(a);
      return;
    }
  }
  k_gather_reduce<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, DST1, HUBF, COMB, false><<<grid, 256, 0, stream>>>(a);
}

// COMB: the rows finish with the EGC combine (egc_combine.hip; one column block, no destination term, no mask)
template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST, bool HAS_ARG, bool MASKED, bool COMB = false>
int launch_all(const Args &a0, int col_blocks, hipStream_t stream) {
  static_assert(!COMB || (!HAS_DST && !MASKED), "the EGC combine finishes plain rows");
  constexpr int ROWS_PER_BLOCK = 256 / LPR;
  Args a = a0;
  a.num_tiles = (a.num_nodes - a.row_begin + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  a.hub_blocks = 0;
  SideStream *side = nullptr;
  // large plans only: on a minibatch-sized graph the launches are ~0.1 ms, have no tail worth hiding, and the
  // fork / join events cost more than they save (measured on cfg3: +20 us per aggregation)
  static const int64_t side_min_edges = [] {
    const char *e = getenv("PTGNN_AMD_SIDE_MIN_EDGES");     // test knob: engage the side streams on small plans too
    return e ? (int64_t)atoll(e) : ((int64_t)1 << 21);
  }();
  if (a.hub_threshold > 0 && a.num_edges >= side_min_edges) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cs);
    side = side_stream(stream, cs == hipStreamCaptureStatusNone);
  }
  bool long_launch = false;
  std::unique_lock<std::mutex> side_lock;
  if (side) side_lock = std::unique_lock<std::mutex>(side->mu);   // fork .. join is one critical section per caller stream
  if (side) {   // fork: hub chunks and long rows each on a side stream of their own, next to the main launch
    PTGNN_HIP(hipEventRecord(side->fork, stream));
    PTGNN_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
    int64_t chunks = (a.num_edges + kHubChunk - 1) / kHubChunk;
    dim3 hgrid((unsigned)(chunks < 1024 ? chunks : 1024), (unsigned)col_blocks);
    k_hub_chunks<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, COMB><<<hgrid, 256, 0, side->stream>>>(a);
    PTGNN_LAUNCH_CHECK();
    PTGNN_HIP(hipEventRecord(side->join, side->stream));
    // long rows: plain rows, and rows with a destination term when there is one edge type (the term is then one
    // row per destination, loaded once -- the DST1 form of the main kernel)
    if constexpr (VEC == 4 && CH == 1 && !MASKED) {
      if (!HAS_DST || a.type_bits == 0) {
        a.long_threshold = kLongRow;
        long_launch = true;
        PTGNN_HIP(hipStreamWaitEvent(side->stream2, side->fork, 0));
        const int64_t lb = (a.num_nodes - a.row_begin + 255) / 256;
        dim3 lgrid((unsigned)(lb < 2048 ? lb : 2048), (unsigned)col_blocks);
        k_long_rows<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, COMB><<<lgrid, 256, 0, side->stream2>>>(a);
        PTGNN_LAUNCH_CHECK();
        PTGNN_HIP(hipEventRecord(side->join2, side->stream2));
      }
    }
  }
  constexpr bool kFuseHub = hub_fuses<CH, HAS_DST, HAS_ARG, MASKED>();
  constexpr bool kHubF = kFuseHub;   // k_gather_reduce's default HUBF, spelled out where COMB follows it
  constexpr bool kFuseSmall = hub_fuses_small<CH, HAS_DST, HAS_ARG, MASKED>();
  // minibatch-sized plans only (below the side streams' threshold): there the list is almost always empty.  A large plan that
  // stays on one stream (side streams switched off or exhausted) keeps the dedicated hub launch with its full grid.
  const bool fuse_small = kFuseSmall && a.num_edges < kFuseDstMaxEdges;
  if ((kFuseHub || fuse_small) && !side && a.hub_threshold > 0 && a.num_edges < side_min_edges) {
    const int64_t chunks = (a.num_edges + kHubChunk - 1) / kHubChunk;
    a.hub_blocks = (int)(((chunks < PTGNN_HUB_FUSED_BLOCKS ? chunks : PTGNN_HUB_FUSED_BLOCKS) + 7) / 8 * 8);
  }
  dim3 grid((unsigned)(xcd_padded_blocks(a.num_tiles) + a.hub_blocks), (unsigned)col_blocks);
  // one edge type (type_bits == 0): the destination term of a row is one row -> the DST1 variant loads it once
  constexpr bool kDst1Variant = VEC == 4 && HAS_DST && !MASKED;
  if constexpr (kFuseSmall) {
    if (a.hub_blocks > 0) {      // the small-plan instantiation that walks the hub list itself
      if (kDst1Variant && a.type_bits == 0)
        launch_main<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, kDst1Variant, true, false>(a, grid, stream);
      else
        launch_main<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, false, true, false>(a, grid, stream);
      PTGNN_LAUNCH_CHECK();
      return PTGNN_AMD_OK;
    }
  }
  if (kDst1Variant && a.type_bits == 0)
    launch_main<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, kDst1Variant, kHubF, COMB>(a, grid, stream);
  else
    launch_main<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, false, kHubF, COMB>(a, grid, stream);
  PTGNN_LAUNCH_CHECK();
  if (side) {   // join: the caller's stream continues once the hub and long rows are written too
    PTGNN_HIP(hipStreamWaitEvent(stream, side->join, 0));
    if (long_launch) PTGNN_HIP(hipStreamWaitEvent(stream, side->join2, 0));
    return PTGNN_AMD_OK;
  }
  if (a.hub_blocks == 0 && a.hub_threshold > 0) {
    // the list length lives on the device: a fixed grid strides over it (zero entries => instant exit)
    int64_t chunks = (a.num_edges + kHubChunk - 1) / kHubChunk;
    dim3 hgrid((unsigned)(chunks < 1024 ? chunks : 1024), (unsigned)col_blocks);
    k_hub_chunks<VEC, LPR, CH, REDUCE, HAS_DST, HAS_ARG, MASKED, COMB><<<hgrid, 256, 0, stream>>>(a);
    PTGNN_LAUNCH_CHECK();
  }
  return PTGNN_AMD_OK;
}

template <int VEC, int LPR, int CH, int REDUCE, bool HAS_DST>
int launch2(const Args &a, int col_blocks, hipStream_t stream) {
  if constexpr (REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN) {
    if (a.argout) return launch_all<VEC, LPR, CH, REDUCE, HAS_DST, true, false>(a, col_blocks, stream);
  }
  return launch_all<VEC, LPR, CH, REDUCE, HAS_DST, false, false>(a, col_blocks, stream);
}

template <int VEC, int LPR, int CH>
int launch1(const Args &a, int reduce, int col_blocks, hipStream_t s) {
  const bool d = a.ydst != nullptr;
  switch (reduce) {
    case PTGNN_AMD_SUM:
      return d ? launch2<VEC, LPR, CH, PTGNN_AMD_SUM, true>(a, col_blocks, s)
               : launch2<VEC, LPR, CH, PTGNN_AMD_SUM, false>(a, col_blocks, s);
    case PTGNN_AMD_MEAN:
      return d ? launch2<VEC, LPR, CH, PTGNN_AMD_MEAN, true>(a, col_blocks, s)
               : launch2<VEC, LPR, CH, PTGNN_AMD_MEAN, false>(a, col_blocks, s);
    case PTGNN_AMD_MAX:
      return d ? launch2<VEC, LPR, CH, PTGNN_AMD_MAX, true>(a, col_blocks, s)
               : launch2<VEC, LPR, CH, PTGNN_AMD_MAX, false>(a, col_blocks, s);
    default:
      return d ? launch2<VEC, LPR, CH, PTGNN_AMD_MIN, true>(a, col_blocks, s)
               : launch2<VEC, LPR, CH, PTGNN_AMD_MIN, false>(a, col_blocks, s);
  }
}

template <int N>
using IC = std::integral_constant<int, N>;

// picks the lane-group geometry for msg_dim; f(IC<VEC>, IC<LPR>, IC<CH>, col_blocks)
template <typename F>
int dispatch_geometry(bool vec4, int msg_dim, bool row_epi, F f) {
  if (vec4) {
    if (msg_dim <= 64) return f(IC<4>{}, IC<16>{}, IC<1>{}, 1);
    if (msg_dim <= 128) return f(IC<4>{}, IC<32>{}, IC<1>{}, 1);
    if (msg_dim <= 256) return f(IC<4>{}, IC<64>{}, IC<1>{}, 1);
    if (msg_dim <= 512) return f(IC<4>{}, IC<64>{}, IC<2>{}, 1);
    PTGNN_REQUIRE(!row_epi, PTGNN_AMD_EUNSUPPORTED,
                  "gather_reduce: LayerNorm epilogue supports msg_dim <= 512 (got %d)", msg_dim);
    return f(IC<4>{}, IC<64>{}, IC<2>{}, (msg_dim + 511) / 512);
  }
  if (msg_dim <= 64) return f(IC<1>{}, IC<64>{}, IC<1>{}, 1);
  if (msg_dim <= 256) return f(IC<1>{}, IC<64>{}, IC<4>{}, 1);
  PTGNN_REQUIRE(!row_epi, PTGNN_AMD_EUNSUPPORTED,
                "gather_reduce: unaligned LayerNorm epilogue supports msg_dim <= 256 (got %d)", msg_dim);
  return f(IC<1>{}, IC<64>{}, IC<4>{}, (msg_dim + 255) / 256);
}

int setup_hub(Args &a, int64_t num_edges, int32_t hub_threshold, const int32_t *hub_entries,
              const int32_t *hub_count, void *hub_ws, size_t hub_ws_bytes, int32_t *hub_tickets,
              bool with_arg) {
  a.num_edges = num_edges;
  a.hub_threshold = 0;
  a.hub_part = nullptr;
  a.hub_arg = nullptr;
  a.hub_tickets = hub_tickets;
  a.hub_entries = hub_entries;
  a.hub_count = hub_count;
  if (hub_ws == nullptr || hub_tickets == nullptr || hub_entries == nullptr || hub_count == nullptr ||
      hub_threshold <= 0 || num_edges <= hub_threshold)
    return PTGNN_AMD_OK;
  PTGNN_REQUIRE(hub_threshold >= 2 * kHubChunk, PTGNN_AMD_EINVAL,
                "gather_reduce: hub_threshold must be 0 or >= %d", 2 * kHubChunk);
  const size_t need = ptgnn_amd_hub_workspace_bytes(num_edges, a.msg_dim, with_arg);
  PTGNN_REQUIRE(hub_ws_bytes >= need, PTGNN_AMD_EWORKSPACE, "gather_reduce: hub workspace %zu < %zu",
                hub_ws_bytes, need);
  const size_t chunks = (size_t)((num_edges + kHubChunk - 1) / kHubChunk);
  char *p = (char *)(((uintptr_t)hub_ws + 255) & ~(uintptr_t)255);
  a.hub_part = (float *)p;
  a.hub_arg = with_arg ? (int32_t *)(p + 2 * chunks * (size_t)a.msg_dim * 4) : nullptr;
  a.hub_threshold = hub_threshold;
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd
