// Opt-in 16-bit matrix-core inputs for the GGNN layer's grouped per-edge GEMM (the edge form's message Linear):
//
//     msg[r, :] = act( rnd(X[src[r], :]) . rnd(W_t)^T )          for every message row r of edge type t
//
// on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation; no bias (the GGNN message Linear has none).  Two launch forms
// over the same kernels:
//   ptgnn_amd_edge_linear16_shared : one row per distinct (type, source) pair; the geometry is the device-resident
//                                    StreamEdgeTable that ptgnn_amd_unique_sources wrote (no host synchronisation)
//   ptgnn_amd_edge_linear16        : one row per edge in type-major order, from host arrays of per-type `src` pointers
// and, for the MLP-MP layer's message Linear (mlpmessagepassing.py:88-98), the per-edge form WITH a target-state half,
//   ptgnn_amd_edge_dst_linear16    : msg[r, :] = act( rnd(X[src[r]]) . rnd(W_t[:, :H])^T + rnd(X[dst[r]]) . rnd(W_t[:, H:])^T )
// and, for the GGNN layer's edge-form TRAINING step (gatedmessagepassing.py:57-61 with its per-edge dropout),
//   ptgnn_amd_edge_masked_linear16 : the per-edge form with the dropout mask from its keep bits (template flag MASK) --
//                                    1: on the gathered input before it is rounded (the forward); 2: on the fp32
//                                    accumulator before the store (the input gradient, over an identity index)
// The DST form runs
// over the same two kernels (template flag DST): the unit carries a second id list, W_t is [M, 2 H], and the chain runs
// over the source half and then over the target half into the same accumulators.  k_edge16_ws takes it at 2 H in
// {128, 256} (its KS = 8 and 16 register budgets; the panel row is [x[src] | x[dst]]), k_edge16 everywhere else.  There
// is no shared-row form: with a target half a message row belongs to one edge.
// Contracts: include/ptgnn_amd.h.  The fp32 pair is ptgnn_amd_edge_linear_shared_f32 / ptgnn_amd_edge_linear_f32
// (edge_gemm.hip, stream_gemm.hip: untouched).
//
// States and messages stay fp32 in HBM; the weights arrive already rounded by the host as ONE 16-bit [T, M, H] stack.
// Operands, the chain, the per-wave tile and the rounded LDS panel: half16.h.
//
// Work unit = 32 consecutive message rows of one type (the table's `unit_off` prefix; its `wg_off` apportioning belongs
// to the fp32 kernel and is not read).  Two kernels, chosen by H and M alone:
//   * k_edge16_ws (H in {64, 128, 256}, M <= 128: the GGNN widths): a workgroup of four waves walks a contiguous run of
//     units; wave s keeps columns [32 s, 32 s + 32) of W_t in registers (H / 16 B fragments, reloaded only when the run
//     crosses into the next type); a unit's 32 gathered rows (a row is one 512-byte request of 32 lanes at H = 128) go
//     through a RoundedPanel.
//   * k_edge16 (every other supported shape): a wave owns a unit x 128 output columns as one wave_tile over the gathered
//     rows, wave-strided over the launch.
//
// Row independence: in both kernels a row's K chain is one accumulator per 32-column tile, zeroed, k ascending in steps
// of 16, on the same rounded operands -- the bits of message row r depend on x[src[r]] and W_t only, not on the launch
// form, the kernel, the row's position in its unit, the number of rows or the workgroup count.  The aggregation that
// follows gives the same bits whichever form ran, as the fp32 pair does.
//
// No atomics, no inline assembly; every store is a plain C++ assignment.
#include <stdlib.h>

#include "half16.h"
#include "stream_gemm.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

struct Edge16Args {
  StreamEdgeTable tab;               // per-edge form: the table by value (src, edge_off, unit_off); shared form: unused
  const StreamEdgeTable *tab_dev;    // shared form: the table in device memory
  const float *x;
  int64_t ld_x, num_rows;            // rows of x: gathered ids are clamped into [0, num_rows)
  const uint16_t *w;                 // [T, M, H], rounded by the host
  int H, M, act;
  float *msg;
  int64_t ld_msg;
  // the masked forms (template flag MASK != 0): the keep bits of the per-edge dropout, [message rows][mask_ld] dwords,
  // bit b of dword c = column 32 c + b of the row the mask covers -- the gathered input row (MASK 1: the forward), the
  // output row (MASK 2: the input gradient) -- and 1 / (1 - p).  Last, so the fields above keep their kernarg offsets.
  const uint32_t *mask;
  int mask_ld;
  float scale;
};

// The id lists are global memory; read out of a table in device memory the pointers would be generic and their loads
// flat (stream_gemm.hip k_stream_edge says what that does to the wait counts).
using GlobalIds = const __attribute__((address_space(1))) int64_t *;

// The 32-row unit `u` of the table: its edge type, its first id, the rows left in the type from there (>= 1) and its
// first message row.  `v_unit` = unit_off[lane] (entries past the last type hold the total): one ballot finds the type.
struct Unit {
  int t;
  GlobalIds ids, dst_ids;            // dst_ids: the target ids of the same rows (the forms with a target-state half only)
  int64_t left, out0;
  // The row of x that message row r of the unit gathers.  Rows past the type's end read its last row (never stored);
  // the ids were range-checked by the plan build and are clamped anyway, so a bad id can never fault.
  __device__ __forceinline__ const float *row_of(GlobalIds list, const float *x, int64_t ld_x, int64_t num_rows,
                                                 int r) const {
    const int64_t id = list[r < left ? r : left - 1];
    return x + (id < 0 ? 0 : (id < num_rows ? id : num_rows - 1)) * ld_x;
  }
  __device__ __forceinline__ const float *row(const float *x, int64_t ld_x, int64_t num_rows, int r) const {
    return row_of(ids, x, ld_x, num_rows, r);
  }
  __device__ __forceinline__ const float *dst_row(const float *x, int64_t ld_x, int64_t num_rows, int r) const {
    return row_of(dst_ids, x, ld_x, num_rows, r);
  }
};
template <bool DST = false>
__device__ __forceinline__ Unit locate(const StreamEdgeTable &tab, int v_unit, int u) {
  Unit q;
  q.t = __popcll(__ballot(v_unit <= u)) - 1;          // last type whose first unit is <= u: the one that owns u
  const int64_t row0 = (int64_t)(u - __builtin_amdgcn_readlane(v_unit, q.t)) * 32;
  const int64_t type_row0 = tab.edge_off[q.t];
  q.left = tab.edge_off[q.t + 1] - type_row0 - row0;
  q.ids = (GlobalIds)tab.src[q.t] + row0;
  if constexpr (DST) q.dst_ids = (GlobalIds)tab.dst[q.t] + row0;
  q.out0 = type_row0 + row0;
  return q;
}

constexpr int kTiles = 4;   // 32-column tiles per wave of k_edge16

// wave_tile (half16.h) with the dropout of MASK 1 on its A operand: the row's keep word of every 32 columns rides with
// the row's two k-steps there, and the kept values are scaled in fp32 BEFORE the one rounding (autocast applies
// nn.Dropout before the 16-bit Linear).  The same chain: one accumulator per tile, zeroed, k ascending in steps of 16.
template <int DT, int TILES>
__device__ __forceinline__ void wave_tile_masked(const float *__restrict__ arow, const uint32_t *__restrict__ mrow,
                                                 float scale, const uint16_t *__restrict__ w, int K, int col0, int tiles,
                                                 f32x16 (&acc)[TILES]) {
  using H = Half16<DT>;
  const int li = frag_li(), hi = frag_hi();
  const float *ap = arow + 8 * hi;
  const uint16_t *bp[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const int tc = t < tiles ? t : tiles - 1;
    bp[t] = w + (int64_t)(col0 + tc * 32 + li) * K + 8 * hi;
    zero(acc[t]);
  }
  for (int kk = 0; kk < K; kk += 32) {
    const uint32_t word = mrow[kk >> 5] >> (8 * hi);   // bit b + j: column kk + b + 8 hi + j
#pragma unroll
    for (int b = 0; b < 32; b += 16) {
      const float4 lo = keep_scaled4(*reinterpret_cast<const float4 *>(ap + kk + b), word, b, scale);
      const float4 up = keep_scaled4(*reinterpret_cast<const float4 *>(ap + kk + b + 4), word, b + 4, scale);
      const f32x8 v = {lo.x, lo.y, lo.z, lo.w, up.x, up.y, up.z, up.w};
      const typename H::vec a = __builtin_convertvector(v, typename H::vec);
#pragma unroll
      for (int t = 0; t < TILES; ++t) acc[t] = H::mfma(a, load8<DT>(bp[t] + kk + b), acc[t]);
    }
  }
}

// DST (both kernels): the message input is [x[src] | x[dst]] and W_t is [M, 2 H] -- one chain over the source half, then
// over the target half, into the same accumulators.
// MASK (both kernels; per-edge form without a target half, no activation): the per-edge dropout of the training step from
// its keep bits.  1: on the gathered input, before it is rounded (the forward); 2: on the fp32 accumulator, before the
// store (the input gradient).  0: no mask -- the code of the unmasked instantiations is what it was.
template <int DT, bool INDIRECT, bool DST = false, int MASK = 0>
__global__ __launch_bounds__(256) void k_edge16(Edge16Args p) {
  const StreamEdgeTable *tabp;
  if constexpr (INDIRECT) tabp = p.tab_dev; else tabp = &p.tab;
  const StreamEdgeTable &tab = *tabp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = frag_li();
  const int v_unit = tab.unit_off[lane];
  const int col_groups = (p.M + 32 * kTiles - 1) / (32 * kTiles);
  const int64_t items = (int64_t)tab.unit_off[kStreamMaxTypes] * col_groups;
  // a wave's items are (unit, column group) pairs, wave-strided over the launch; no barrier in this kernel
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < items; i += (int64_t)gridDim.x * 4) {
    const Unit q = locate<DST>(tab, v_unit, (int)(i / col_groups));
    const int col0 = (int)(i % col_groups) * (32 * kTiles);
    const int tiles = (p.M - col0) / 32 < kTiles ? (p.M - col0) / 32 : kTiles;   // >= 1

    f32x16 acc[kTiles];
    if constexpr (DST) {
      const uint16_t *w = p.w + (int64_t)q.t * p.M * (2 * p.H);
#pragma unroll
      for (int n = 0; n < kTiles; ++n) zero(acc[n]);
      wave_tile_more<DT>(q.row(p.x, p.ld_x, p.num_rows, li), w, 2 * p.H, p.H, col0, tiles, acc);
      wave_tile_more<DT>(q.dst_row(p.x, p.ld_x, p.num_rows, li), w + p.H, 2 * p.H, p.H, col0, tiles, acc);
    } else if constexpr (MASK == 1) {   // the mask row of a row past the type's end: the last row's, like the gather
      const uint32_t *mrow = p.mask + (q.out0 + (li < q.left ? li : q.left - 1)) * p.mask_ld;
      wave_tile_masked<DT>(q.row(p.x, p.ld_x, p.num_rows, li), mrow, p.scale, p.w + (int64_t)q.t * p.M * p.H, p.H, col0,
                           tiles, acc);
    } else {
      wave_tile<DT>(q.row(p.x, p.ld_x, p.num_rows, li), p.w + (int64_t)q.t * p.M * p.H, p.H, col0, tiles, acc);
    }
#pragma unroll
    for (int n = 0; n < kTiles; ++n) {
      if (n < tiles) {
        const int col = col0 + n * 32 + li;
        for_frag_rows(q.out0, q.out0 + q.left, [&](int r, int64_t row) {
          if constexpr (MASK == 2)      // the keep word of this row's 32-column tile; this lane's column is bit li
            p.msg[row * p.ld_msg + col] = keep_scaled(acc[n][r], p.mask[row * p.mask_ld + (col >> 5)], li, p.scale);
          else
            p.msg[row * p.ld_msg + col] = act_runtime(acc[n][r], p.act);
        });
      }
    }
  }
}

template <int DT, int KS, bool INDIRECT, bool DST = false, int MASK = 0>
__global__ __launch_bounds__(256) void k_edge16_ws(Edge16Args p) {
  using Hf = Half16<DT>;
  using vec = typename Hf::vec;
  constexpr int H = 16 * KS;             // the K of the chain = the panel's width; DST: 2 x state_dim
  RoundedPanel<DT, 32, H> panel;

  const StreamEdgeTable *tabp;
  if constexpr (INDIRECT) tabp = p.tab_dev; else tabp = &p.tab;
  const StreamEdgeTable &tab = *tabp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = frag_li(), hi = frag_hi();
  const int v_unit = tab.unit_off[lane];
  const int64_t total = tab.unit_off[kStreamMaxTypes];
  // a contiguous run of the type-major unit order per workgroup: few type changes, and no table of its own to balance
  const int u_begin = (int)(blockIdx.x * total / gridDim.x), u_end = (int)((blockIdx.x + 1) * total / gridDim.x);
  if (u_begin >= u_end) return;          // whole workgroup: before any barrier
  const int j = wave * 32 + li;          // this lane's output column
  const bool active = wave * 32 < p.M;   // M < 128: the waves past the last column slice only gather

  // The unit's gathered rows.  Operands by value: read through a reference to `p` inside the closure, the clamp of the
  // first gather compiles to a branch per id and the four id -> row chains of the prologue run one after the other.
  const float *const x = p.x;
  const int64_t ld_x = p.ld_x, num_rows = p.num_rows;
  auto rows_of = [=](const Unit &q) {
    return [=](int r, int c) {
      if constexpr (DST)                 // a panel row is [x[src] | x[dst]]; a float4 never straddles (H / 2 % 4 == 0)
        return c < H / 2 ? q.row(x, ld_x, num_rows, r) + c : q.dst_row(x, ld_x, num_rows, r) + (c - H / 2);
      else
        return q.row(x, ld_x, num_rows, r) + c;
    };
  };

  // MASK 1: one keep word per staged float4 (8 threads share a word: one request) rides with the unit's rows and is
  // consumed while they are rounded into the panel -- the kept values scaled in fp32 before the one rounding.
  using Panel = RoundedPanel<DT, 32, H>;
  const uint32_t *const mask = p.mask;
  const int mask_ld = p.mask_ld;
  const float scale = p.scale;
  uint32_t mw[MASK == 1 ? Panel::NV : 1];
  auto fetch_mask = [&](const Unit &q) {
#pragma unroll
    for (int i = 0; i < Panel::NV; ++i) {
      const int v = threadIdx.x + i * 256, r = v / Panel::RV, c = (v % Panel::RV) * 4;
      mw[i] = mask[(q.out0 + (r < q.left ? r : q.left - 1)) * mask_ld + (c >> 5)];   // past the end: the last row's
    }
  };
  auto drop = [&](int i, int, int c, float4 &v) { v = keep_scaled4(v, mw[i], c & 31, scale); };

  vec bw[KS];                            // columns j of W_t, all of K
  int t_loaded = -1;
  Unit cur = locate<DST>(tab, v_unit, u_begin);
  if constexpr (MASK == 1) {
    panel.fetch(rows_of(cur));
    fetch_mask(cur);
    panel.edit(drop);
    panel.start();
  } else {
    panel.prime(rows_of(cur));
  }
  for (int u = u_begin; u < u_end; ++u) {
    const Unit nxt = locate<DST>(tab, v_unit, u + 1 < u_end ? u + 1 : u);   // no branch around the loads: the last trip
    panel.fetch(rows_of(nxt));                                          // re-reads its own unit
    if constexpr (MASK == 1) fetch_mask(nxt);
    if (active) {
      if (cur.t != t_loaded) {           // wave-uniform
        t_loaded = cur.t;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bw[ks] = load8<DT>(p.w + ((int64_t)cur.t * p.M + j) * H + ks * 16 + 8 * hi);
      }
      // MASK 2: lane l asks for the keep word of the unit's row l & 31 (word `wave` of a row: columns 32 wave ..; a row past
      // the type's end reads the last row's) before the chain -- one register; the fragment epilogue reads the words of
      // its 16 rows out of the lanes (register r is row frag_row(r, 0) in the lower lane half, 4 further in the upper)
      uint32_t mrow = 0;
      if constexpr (MASK == 2) mrow = mask[(cur.out0 + (li < cur.left ? li : cur.left - 1)) * mask_ld + wave];
      f32x16 acc;
      zero(acc);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = Hf::mfma(panel.frag(li, ks), bw[ks], acc);
      for_frag_rows(cur.out0, cur.out0 + cur.left, [&](int r, int64_t row) {
        if constexpr (MASK == 2) {
          const uint32_t lo = __builtin_amdgcn_readlane(mrow, frag_row(r, 0)), up = __builtin_amdgcn_readlane(mrow, frag_row(r, 1));
          p.msg[row * p.ld_msg + j] = keep_scaled(acc[r], hi ? up : lo, li, scale);
        } else {
          p.msg[row * p.ld_msg + j] = act_runtime(acc[r], p.act);
        }
      });
    }
    if constexpr (MASK == 1) panel.edit(drop);
    panel.flip();
    cur = nxt;
  }
}

bool shape_ok(int32_t state_dim, int32_t msg_dim, int32_t num_types) {
  return state_dim > 0 && state_dim % 32 == 0 && state_dim <= 1024 && msg_dim > 0 && msg_dim % 32 == 0 &&
         msg_dim <= 1024 && num_types >= 2 && num_types <= kStreamMaxTypes;
}

int env_int(const char *name, int fallback, int lo, int hi) {   // developer A/B knobs
  if (const char *e = getenv(name)) {
    const int v = atoi(e);
    if (v >= lo && v <= hi) return v;
  }
  return fallback;
}

// the argument checks the entries share; everything here answers before anything touches the device.  `who`: "" or
// " dst:" -- the messages of the entry with a target-state half start "edge_linear16: dst:"
int check_operands(const char *who, const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim, const void *w,
                   int32_t msg_dim, const float *msg, int64_t ld_msg) {
  PTGNN_REQUIRE(x && w && msg, PTGNN_AMD_EINVAL, "edge_linear16:%s null pointer", who);
  PTGNN_REQUIRE(num_rows > 0 && ld_x >= state_dim && ld_msg >= msg_dim, PTGNN_AMD_EINVAL,
                "edge_linear16:%s num_rows must be positive, ld_x >= state_dim and ld_msg >= msg_dim", who);
  PTGNN_REQUIRE(rows16(x, ld_x) && aligned16(w) && aligned4(msg), PTGNN_AMD_EUNSUPPORTED,
                "edge_linear16:%s x and w must be 16-byte aligned with ld_x %% 4 == 0 (ld_x=%lld), msg float-aligned",
                who, (long long)ld_x);
  return PTGNN_AMD_OK;
}

int check_shape(const char *who, int32_t state_dim, int32_t num_types, int32_t msg_dim, int act, int dtype) {
  PTGNN_REQUIRE(num_types > 0 && state_dim > 0 && msg_dim > 0, PTGNN_AMD_EINVAL, "edge_linear16:%s bad sizes", who);
  PTGNN_REQUIRE(act >= 0 && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "edge_linear16:%s bad act", who);
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "edge_linear16:%s dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16",
                who, dtype);
  PTGNN_REQUIRE(shape_ok(state_dim, msg_dim, num_types), PTGNN_AMD_EUNSUPPORTED,
                "edge_linear16:%s state_dim=%d msg_dim=%d num_types=%d: needs both widths %% 32 == 0 and <= 1024, "
                "2 <= num_types <= %d", who, state_dim, msg_dim, num_types, kStreamMaxTypes);
  return PTGNN_AMD_OK;
}

// The per-edge entries' table from HOST arrays of per-type id pointers and counts; `dst_per_type` null: no target half.
// `units`: the 32-row units of the launch (0: nothing to launch).
int host_table(const char *who, const int64_t *const *src_per_type, const int64_t *const *dst_per_type,
               const int64_t *edges_per_type, int32_t num_types, bool with_dst, StreamEdgeTable &tab, int64_t &units) {
  PTGNN_REQUIRE(edges_per_type, PTGNN_AMD_EINVAL, "edge_linear16:%s null edge counts", who);
  tab.num_types = num_types;
  units = 0;
  for (int t = 0; t < num_types; ++t) {
    const int64_t n = edges_per_type[t];
    PTGNN_REQUIRE(n >= 0, PTGNN_AMD_EINVAL, "edge_linear16:%s negative edge count of type %d", who, t);
    PTGNN_REQUIRE(n == 0 || (src_per_type && src_per_type[t]), PTGNN_AMD_EINVAL,
                  "edge_linear16:%s null source ids of type %d", who, t);
    PTGNN_REQUIRE(!with_dst || n == 0 || (dst_per_type && dst_per_type[t]), PTGNN_AMD_EINVAL,
                  "edge_linear16:%s null target ids of type %d", who, t);
    tab.src[t] = n ? src_per_type[t] : nullptr;
    tab.dst[t] = n && with_dst ? dst_per_type[t] : nullptr;
    tab.edge_off[t + 1] = tab.edge_off[t] + n;
    units += (n + 31) / 32;
    PTGNN_REQUIRE(units < ((int64_t)1 << 30), PTGNN_AMD_EUNSUPPORTED, "edge_linear16:%s too many 32-row units", who);
    tab.unit_off[t + 1] = (int32_t)units;
  }
  for (int t = num_types + 1; t <= kStreamMaxTypes; ++t) {   // the kernels fetch the prefix one entry per lane and search
    tab.unit_off[t] = (int32_t)units;                        // it with a ballot: entries past the last type hold the total
    tab.edge_off[t] = tab.edge_off[num_types];
  }
  return PTGNN_AMD_OK;
}

// Workgroups of a weight-stationary instance that one CU holds at once (registers and LDS decide; asked once).  The
// launch is ONE such round: measured at the cfg3 layer shapes, any grid that needs a partly filled second round loses
// 15 - 20 % to it (profiles/edge_inputs_notes.md).
template <int DT, int KS, bool INDIRECT, bool DST, int MASK>
int ws_resident_per_cu() {
  static const int per_cu = [] {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_edge16_ws<DT, KS, INDIRECT, DST, MASK>, 256, 0) != hipSuccess ||
        n < 1) {
      (void)hipGetLastError();
      n = 2;
    }
    return n;
  }();
  return per_cu;
}

// `units` < 0: unknown on the host (shared form) -- the launch is sized for the device, workgroups without units leave
// DST: the chain is 2 H long, so the weight-stationary register budgets (KS = 8, 16) hold H in {64, 128}
template <bool INDIRECT, bool DST = false, int MASK = 0>
int launch(const Edge16Args &p, int dtype, int64_t units, hipStream_t st) {
  const int64_t cus = num_compute_units();
  const int k = DST ? 2 * p.H : p.H;
  const bool ws = (k == 128 || k == 256 || (!DST && k == 64)) && p.M <= 128 &&
                  env_int("PTGNN_AMD_EDGE16_WS", 1, 0, 1) == 1;
  if (ws) {
    const int knob = env_int("PTGNN_AMD_EDGE16_WGS", 0, 0, 16);   // workgroups per CU; 0: one resident round
    with_dtype(dtype, [&](auto dt) {
      auto run = [&](auto ks) {
        constexpr int DT = decltype(dt)::value, KS = decltype(ks)::value;
        int64_t grid = cus * (knob ? knob : ws_resident_per_cu<DT, KS, INDIRECT, DST, MASK>());
        if (units >= 0 && units < grid) grid = units;
        k_edge16_ws<DT, KS, INDIRECT, DST, MASK><<<(unsigned)grid, 256, 0, st>>>(p);
      };
      if constexpr (DST) with_case<8, 16>(k / 16, run); else with_case<4, 8, 16>(k / 16, run);
    });
  } else {
    const int col_groups = (p.M + 32 * kTiles - 1) / (32 * kTiles);
    int64_t grid = cus * 8;
    if (units >= 0 && (units * col_groups + 3) / 4 < grid) grid = (units * col_groups + 3) / 4;
    with_dtype(dtype,
               [&](auto dt) { k_edge16<decltype(dt)::value, INDIRECT, DST, MASK><<<(unsigned)grid, 256, 0, st>>>(p); });
  }
  PTGNN_LAUNCH_CHECK();
  count_launch(MASK ? PTGNN_AMD_KERNEL_EDGE16_MASKED
                    : (DST ? PTGNN_AMD_KERNEL_EDGE16_DST
                           : (INDIRECT ? PTGNN_AMD_KERNEL_EDGE16_SHARED : PTGNN_AMD_KERNEL_EDGE16)));
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_edge_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype) {
  return dtype_ok(dtype) && shape_ok(state_dim, msg_dim, num_types) ? 1 : 0;
}

extern "C" int ptgnn_amd_edge_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                       const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                       const void *w, int32_t num_types, int32_t msg_dim, int act, int dtype,
                                       float *msg, int64_t ld_msg, void *stream_) {
  if (const int rc = check_shape("", state_dim, num_types, msg_dim, act, dtype)) return rc;
  Edge16Args p{};
  int64_t units = 0;
  if (const int rc = host_table("", src_per_type, nullptr, edges_per_type, num_types, false, p.tab, units)) return rc;
  if (units == 0) return PTGNN_AMD_OK;                       // no rows: no launch
  if (const int rc = check_operands("", x, ld_x, num_rows, state_dim, w, msg_dim, msg, ld_msg)) return rc;
  p.x = x; p.ld_x = ld_x; p.num_rows = num_rows; p.w = static_cast<const uint16_t *>(w);
  p.H = state_dim; p.M = msg_dim; p.act = act; p.msg = msg; p.ld_msg = ld_msg;
  return launch<false>(p, dtype, units, (hipStream_t)stream_);
}

extern "C" int ptgnn_amd_edge_masked_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype,
                                                        int dropout_mode) {
  // the mask covers state_dim (mode 1) or msg_dim (mode 2) columns in 32-bit words: both are multiples of 32 already
  return (dropout_mode == 1 || dropout_mode == 2) && dtype_ok(dtype) && shape_ok(state_dim, msg_dim, num_types) ? 1 : 0;
}

extern "C" int ptgnn_amd_edge_masked_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                              const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                              const void *w, int32_t num_types, int32_t msg_dim, int dtype, float *msg,
                                              int64_t ld_msg, int dropout_mode, float dropout_p,
                                              const uint32_t *mask_bits, void *stream_) {
  PTGNN_REQUIRE(dropout_mode >= 0 && dropout_mode <= 2 && dropout_p >= 0.f && dropout_p < 1.f, PTGNN_AMD_EINVAL,
                "edge_linear16: masked: bad dropout mode / probability");
  if (dropout_p == 0.f || mask_bits == nullptr) dropout_mode = 0;
  if (const int rc = check_shape(" masked:", state_dim, num_types, msg_dim, PTGNN_AMD_ACT_NONE, dtype)) return rc;
  Edge16Args p{};
  int64_t units = 0;
  if (const int rc = host_table(" masked:", src_per_type, nullptr, edges_per_type, num_types, false, p.tab, units))
    return rc;
  if (units == 0) return PTGNN_AMD_OK;                       // no rows: no launch
  if (const int rc = check_operands(" masked:", x, ld_x, num_rows, state_dim, w, msg_dim, msg, ld_msg)) return rc;
  PTGNN_REQUIRE(dropout_mode == 0 || aligned4(mask_bits), PTGNN_AMD_EUNSUPPORTED,
                "edge_linear16: masked: mask_bits must be 4-byte aligned");
  p.x = x; p.ld_x = ld_x; p.num_rows = num_rows; p.w = static_cast<const uint16_t *>(w);
  p.H = state_dim; p.M = msg_dim; p.act = PTGNN_AMD_ACT_NONE; p.msg = msg; p.ld_msg = ld_msg;
  if (dropout_mode == 0) return launch<false>(p, dtype, units, (hipStream_t)stream_);   // the unmasked launch, its bits
  p.mask = mask_bits;
  p.mask_ld = (dropout_mode == 2 ? msg_dim : state_dim) / 32;
  p.scale = 1.0f / (1.0f - dropout_p);
  return dropout_mode == 1 ? launch<false, false, 1>(p, dtype, units, (hipStream_t)stream_)
                           : launch<false, false, 2>(p, dtype, units, (hipStream_t)stream_);
}

extern "C" int ptgnn_amd_edge_dst_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype) {
  return dtype_ok(dtype) && shape_ok(state_dim, msg_dim, num_types) ? 1 : 0;
}

extern "C" int ptgnn_amd_edge_dst_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                           const int64_t *const *src_per_type, const int64_t *const *dst_per_type,
                                           const int64_t *edges_per_type, const void *w, int32_t num_types,
                                           int32_t msg_dim, int act, int dtype, float *msg, int64_t ld_msg,
                                           void *stream_) {
  if (const int rc = check_shape(" dst:", state_dim, num_types, msg_dim, act, dtype)) return rc;
  Edge16Args p{};
  int64_t units = 0;
  if (const int rc = host_table(" dst:", src_per_type, dst_per_type, edges_per_type, num_types, true, p.tab, units))
    return rc;
  if (units == 0) return PTGNN_AMD_OK;                       // no rows: no launch
  if (const int rc = check_operands(" dst:", x, ld_x, num_rows, state_dim, w, msg_dim, msg, ld_msg)) return rc;
  p.x = x; p.ld_x = ld_x; p.num_rows = num_rows; p.w = static_cast<const uint16_t *>(w);
  p.H = state_dim; p.M = msg_dim; p.act = act; p.msg = msg; p.ld_msg = ld_msg;
  return launch<false, true>(p, dtype, units, (hipStream_t)stream_);
}

extern "C" int ptgnn_amd_edge_linear16_shared(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                              const void *edge_table, const void *w, int32_t num_types,
                                              int32_t msg_dim, int act, int dtype, float *msg, int64_t ld_msg,
                                              void *stream_) {
  if (const int rc = check_shape("", state_dim, num_types, msg_dim, act, dtype)) return rc;
  PTGNN_REQUIRE(edge_table, PTGNN_AMD_EINVAL, "edge_linear16: shared: null edge table");
  if (const int rc = check_operands("", x, ld_x, num_rows, state_dim, w, msg_dim, msg, ld_msg)) return rc;
  // the table's (type, source) keys are int32 (ptgnn_amd_unique_sources): no table exists beyond that
  PTGNN_REQUIRE(num_rows * num_types < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "edge_linear16: shared: too many (type, source) pairs (%lld rows x %d types)", (long long)num_rows,
                num_types);
  Edge16Args p{};
  p.tab_dev = static_cast<const StreamEdgeTable *>(edge_table);
  p.x = x; p.ld_x = ld_x; p.num_rows = num_rows; p.w = static_cast<const uint16_t *>(w);
  p.H = state_dim; p.M = msg_dim; p.act = act; p.msg = msg; p.ld_msg = ld_msg;
  return launch<true>(p, dtype, -1, (hipStream_t)stream_);
}
