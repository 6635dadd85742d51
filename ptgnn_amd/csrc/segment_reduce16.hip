// The aggregation of the GGNN edge-form TRAINING step over 16-bit message rows, and its backward
// (the opt-in `half_messages(training=True)` of ptgnn_amd/precision.py):
//
//   ptgnn_amd_segment_reduce16 : out[v, :] = reduce over the CSR slots i of v of float(rows16[col[i], :])   fp32 [N, M]
//                                arg[v, c] = the slot that won column c (max / min), -1 for an empty row     int32 [N, M]
//   ptgnn_amd_segment_spread16 : grad_msg16[perm[s], :] = rnd(source(s))                                    16-bit [E, M]
//                                source = g[row(s)] (sum), g[row(s)] * (1 / deg) (mean),
//                                         arg[row(s), c] == s ? g[row(s), c] : +0 (max / min)
// Contracts + reference lines: include/ptgnn_amd.h.  The fp32 pair (ptgnn_amd_gather_reduce_f32 with an argout,
// ptgnn_amd_segment_spread_f32) is untouched.
//
// Aggregation.  The mapping of gather_reduce16.hip, with a slot index beside every accumulator: a lane owns 8 consecutive
// columns (one 16-byte load = 8 values), a destination row a group of LPR lanes (the power of two >= M / 8 in
// {4, 8, 16, 32}); the values become fp32 in registers (gather_reduce16.h widen2) and fold in CSR order; the slot loop
// runs in groups of 8 slots with all 8 row loads (128 B per lane) issued before the first is used and the next group's
// `col` entries requested behind them.
// The tie rule is ptgnn_amd_gather_reduce_f32's (gather_reduce_core.h RowOp::fold): a candidate replaces the accumulator
// only when it is STRICTLY better, candidates meet it in ascending slot order, so the EARLIEST slot of a tie keeps the
// arg; the accumulator starts at -FLT_MAX / +FLT_MAX with arg -1, so a value that does not beat the start (-inf for max)
// leaves -1 too, as there.  Ties are the normal case on 16-bit rows.  Per path:
//   * rows up to `hub_threshold` in-edges -- the rows beyond kLongRow (256) included, which the fp32 walk hands to a launch
//     of their own -- fold serially on their lane group: ascending slots, strict compare.  A short row or a tail is one
//     more group of 8 with its indices clamped to the row's last slot: a duplicate is that slot's own value met AFTER it,
//     never strictly better, so it cannot take the arg (the sums zero it).
//   * HUB rows (more in-edges) are folded by their whole workgroup afterwards: lane group q takes the q-th CONTIGUOUS run
//     of slots, partial values and args meet in LDS and group 0 folds them in run order with the same strict compare --
//     runs ascend in slot, so the earliest slot of a tie still wins; an empty run holds the start value and arg -1 and
//     never wins.  One launch, fixed order, deterministic.  The fold order of a hub row's SUM differs from the serial order
//     (fp32 rounding only), as the fp32 hub rows' does.
//
// Spread.  Element-parallel: a lane owns 8 consecutive columns of one CSR slot -- two float4 loads of the gradient row
// (rows of a slot run are adjacent: row-sequential reads), two int4 of the arg row for max / min, ONE 16-byte store of the
// 8 rounded values into message row perm[s].  Every message row is written exactly once as a whole row: nothing to zero,
// nothing to accumulate.  The mean's 1 / deg is one IEEE fp32 division per lane and one fp32 multiply per value, BEFORE
// the one rounding (round to nearest even: fptrunc, what tensor.to(dtype) does).  No [N, M] temporary.
//
// No atomics, no inline assembly; every store is a plain C++ assignment.
#include <float.h>

#include "common.h"
#include "gather_reduce16.h"

namespace ptgnn_amd {
namespace {

struct SegArgs16 {
  const uint16_t *rows;      // 16-bit message rows, leading dimension ld (elements)
  int64_t ld;
  const int32_t *rowptr;
  const int32_t *col;        // slot -> message row
  int32_t msg_dim;
  int64_t num_nodes;
  int64_t num_tiles;
  int32_t hub_threshold;     // rows with more in-edges are folded by their whole workgroup (0 = none)
  float *out;
  int64_t ld_out;
  int32_t *argout;           // [num_nodes, msg_dim], max / min with HAS_ARG
};

// One lane's share (8 columns from `colx`) of one destination row, or of one run of a hub row.
template <int DT, int REDUCE, bool HAS_ARG>
struct SegRow16 {
  static constexpr bool kMinMax = REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN;
  static constexpr float kInit = REDUCE == PTGNN_AMD_MAX ? -FLT_MAX : (REDUCE == PTGNN_AMD_MIN ? FLT_MAX : 0.f);
  float acc[8];
  int32_t arg[HAS_ARG ? 8 : 1];

  __device__ __forceinline__ SegRow16() {
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = kInit;
    if constexpr (HAS_ARG) {
#pragma unroll
      for (int v = 0; v < 8; ++v) arg[v] = -1;
    }
  }

  // one candidate per column, all of slot `slot`: strictly better replaces, so the earlier slot of a tie stays
  __device__ __forceinline__ void fold(const float (&m)[8], int32_t slot) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if constexpr (kMinMax) {
        const bool better = REDUCE == PTGNN_AMD_MAX ? m[v] > acc[v] : m[v] < acc[v];
        acc[v] = better ? m[v] : acc[v];
        if constexpr (HAS_ARG) arg[v] = better ? slot : arg[v];
      } else {
        acc[v] += m[v];
      }
    }
  }

  // a partial of LATER slots than ours (the hub combine, run order): the same strict compare, its own slot per column
  __device__ __forceinline__ void fold_partial(const float (&m)[8], const int32_t (&ma)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if constexpr (kMinMax) {
        const bool better = REDUCE == PTGNN_AMD_MAX ? m[v] > acc[v] : m[v] < acc[v];
        acc[v] = better ? m[v] : acc[v];
        if constexpr (HAS_ARG) arg[v] = better ? ma[v] : arg[v];
      } else {
        acc[v] += m[v];
      }
    }
  }

  // slots [beg, end) in CSR order, groups of 8, one round trip per group
  __device__ __forceinline__ void reduce(const SegArgs16 &a, int colx, int beg, int end) {
    if (beg >= end) return;
    const int last = end - 1;
    const uint16_t *base = a.rows + colx;
    int32_t pk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pk[u] = a.col[beg + u < last ? beg + u : last];
    for (int i = beg; i < end; i += 8) {
      u32x4 raw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) raw[u] = *reinterpret_cast<const u32x4 *>(base + (int64_t)pk[u] * a.ld);
#pragma unroll
      for (int u = 0; u < 8; ++u) {       // the next group's col entries ride behind this group's rows
        const int idx = i + 8 + u;
        pk[u] = a.col[idx < last ? idx : last];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool valid = i + u < end;
        float m[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) widen2<DT>(raw[u][d], m[2 * d], m[2 * d + 1]);
        if constexpr (!kMinMax) {
#pragma unroll
          for (int v = 0; v < 8; ++v) m[v] = valid ? m[v] : 0.f;   // a clamped duplicate adds nothing
        }
        fold(m, valid ? i + u : last);     // max / min: a duplicate of the last slot comes after it and is never better
      }
    }
  }

  // mean / empty-segment rule, then the row's 8 columns as two float4 (+ two int4 of args)
  __device__ __forceinline__ void finish_and_store(float *orow, int32_t *arow, int deg) {
    if constexpr (REDUCE == PTGNN_AMD_MEAN) {
      const float cnt = (float)(deg < 1 ? 1 : deg);
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = acc[v] / cnt;
    }
    if (kMinMax && deg == 0) {
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = 0.f;                    // torch_scatter: empty segment -> 0 (arg stays -1)
    }
    *reinterpret_cast<float4 *>(orow) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4 *>(orow + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    if constexpr (HAS_ARG) {
      *reinterpret_cast<int4 *>(arow) = make_int4(arg[0], arg[1], arg[2], arg[3]);
      *reinterpret_cast<int4 *>(arow + 4) = make_int4(arg[4], arg[5], arg[6], arg[7]);
    }
  }
};

template <int DT, int LPR, int REDUCE, bool HAS_ARG>
__global__ __launch_bounds__(256) void k_segment_reduce16(SegArgs16 a) {
  constexpr int G = 256 / LPR;           // destination rows (lane groups) per workgroup
  constexpr int W = LPR * 8;             // columns a lane group spans (>= msg_dim)
  __shared__ __attribute__((aligned(16))) float part[G * W];
  __shared__ __attribute__((aligned(16))) int32_t parg[HAS_ARG ? G * W : 4];
  __shared__ int long_flag[G];

  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;       // whole workgroup: before any barrier
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int colx = g * 8;
  const bool active = colx < a.msg_dim;  // lanes past M are idle
  const int64_t row0 = tile * G;
  const int64_t row = row0 + grp;

  int beg = 0, end = 0;
  if (row < a.num_nodes) {
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
  }
  const bool is_long = a.hub_threshold > 0 && end - beg > a.hub_threshold;
  if (row < a.num_nodes && !is_long && active) {
    SegRow16<DT, REDUCE, HAS_ARG> op;
    op.reduce(a, colx, beg, end);
    op.finish_and_store(a.out + row * a.ld_out + colx, HAS_ARG ? a.argout + row * a.msg_dim + colx : nullptr, end - beg);
  }
  if (!__syncthreads_or(is_long ? 1 : 0)) return;   // no hub row in this tile: the usual case

  if (g == 0) long_flag[grp] = is_long ? 1 : 0;
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < G; ++q) {
    if (!long_flag[q]) continue;         // workgroup-uniform
    const int64_t r = row0 + q;
    const int rbeg = a.rowptr[r], rend = a.rowptr[r + 1];
    // lane group `grp` folds the grp-th contiguous run of the row, so the combine order below is slot order
    const int per = (rend - rbeg + G - 1) / G;
    const int64_t first = (int64_t)rbeg + (int64_t)grp * per;
    const int b = first < rend ? (int)first : rend;
    const int e = first + per < rend ? (int)(first + per) : rend;
    SegRow16<DT, REDUCE, HAS_ARG> op;
    if (active) op.reduce(a, colx, b, e);
    if (grp != 0) {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        part[grp * W + colx + v] = op.acc[v];
        if constexpr (HAS_ARG) parg[grp * W + colx + v] = op.arg[v];
      }
    }
    __syncthreads();
    if (grp == 0 && active) {
      for (int p = 1; p < G; ++p) {      // fixed combine order, runs ascending in slot => deterministic, earliest tie wins
        float m[8];
        int32_t ma[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const float4 lo = *reinterpret_cast<const float4 *>(part + p * W + colx);
        const float4 hi = *reinterpret_cast<const float4 *>(part + p * W + colx + 4);
        m[0] = lo.x; m[1] = lo.y; m[2] = lo.z; m[3] = lo.w;
        m[4] = hi.x; m[5] = hi.y; m[6] = hi.z; m[7] = hi.w;
        if constexpr (HAS_ARG) {
          const int4 alo = *reinterpret_cast<const int4 *>(parg + p * W + colx);
          const int4 ahi = *reinterpret_cast<const int4 *>(parg + p * W + colx + 4);
          ma[0] = alo.x; ma[1] = alo.y; ma[2] = alo.z; ma[3] = alo.w;
          ma[4] = ahi.x; ma[5] = ahi.y; ma[6] = ahi.z; ma[7] = ahi.w;
        }
        op.fold_partial(m, ma);            // an empty run holds the initial value: it changes nothing
      }
      op.finish_and_store(a.out + r * a.ld_out + colx, HAS_ARG ? a.argout + r * a.msg_dim + colx : nullptr, rend - rbeg);
    }
    __syncthreads();                      // group 0 is done with `part` before the next long row fills it
  }
}

template <int DT, int LPR>
void launch_reduce(const SegArgs16 &a0, int reduce, hipStream_t st) {
  SegArgs16 a = a0;
  constexpr int G = 256 / LPR;
  a.num_tiles = (a.num_nodes + G - 1) / G;
  const unsigned grid = (unsigned)xcd_padded_blocks(a.num_tiles);
  const bool with_arg = a.argout != nullptr;
  switch (reduce) {
    case PTGNN_AMD_SUM: k_segment_reduce16<DT, LPR, PTGNN_AMD_SUM, false><<<grid, 256, 0, st>>>(a); break;
    case PTGNN_AMD_MEAN: k_segment_reduce16<DT, LPR, PTGNN_AMD_MEAN, false><<<grid, 256, 0, st>>>(a); break;
    case PTGNN_AMD_MAX:
      if (with_arg) k_segment_reduce16<DT, LPR, PTGNN_AMD_MAX, true><<<grid, 256, 0, st>>>(a);
      else k_segment_reduce16<DT, LPR, PTGNN_AMD_MAX, false><<<grid, 256, 0, st>>>(a);
      break;
    default:
      if (with_arg) k_segment_reduce16<DT, LPR, PTGNN_AMD_MIN, true><<<grid, 256, 0, st>>>(a);
      else k_segment_reduce16<DT, LPR, PTGNN_AMD_MIN, false><<<grid, 256, 0, st>>>(a);
      break;
  }
}

template <int DT>
void launch_dtype(const SegArgs16 &a, int reduce, hipStream_t st) {
  const int lanes = a.msg_dim / 8;
  if (lanes <= 4) launch_reduce<DT, 4>(a, reduce, st);
  else if (lanes <= 8) launch_reduce<DT, 8>(a, reduce, st);
  else if (lanes <= 16) launch_reduce<DT, 16>(a, reduce, st);
  else launch_reduce<DT, 32>(a, reduce, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// spread
// ---------------------------------------------------------------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x8 = __attribute__((ext_vector_type(8))) float;

template <int DT>
__device__ __forceinline__ u32x4 round8(const f32x8 &v) {
  if constexpr (DT == PTGNN_AMD_HALF_BF16) return __builtin_bit_cast(u32x4, __builtin_convertvector(v, bf16x8));
  else return __builtin_bit_cast(u32x4, __builtin_convertvector(v, f16x8));
}

// MODE 0: sum; 1: mean (scale by 1 / deg); 2: max / min (arg).  `q` = dim / 8 lanes per slot, `spb` = 256 / q slots per
// workgroup (the lanes past spb * q idle: q = 12 leaves 4).
template <int DT, int MODE>
__global__ __launch_bounds__(256) void k_segment_spread16(const float *__restrict__ grad, int64_t ld_grad,
                                                          const int32_t *__restrict__ arg,
                                                          const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ slot_row,
                                                          const int32_t *__restrict__ perm, int64_t num_slots, int dim,
                                                          int q, int spb, uint16_t *__restrict__ out, int64_t ld_out) {
  const int local = (int)threadIdx.x / q;
  const int c = ((int)threadIdx.x - local * q) * 8;
  const int64_t s = (int64_t)blockIdx.x * spb + local;
  if (local >= spb || s >= num_slots) return;
  const int64_t row = slot_row[s];
  const int64_t e = perm[s];
  const float *gp = grad + row * ld_grad + c;
  const float4 lo = *reinterpret_cast<const float4 *>(gp), up = *reinterpret_cast<const float4 *>(gp + 4);
  f32x8 v = {lo.x, lo.y, lo.z, lo.w, up.x, up.y, up.z, up.w};
  if constexpr (MODE == 1) {
    const int deg = rowptr[row + 1] - rowptr[row];      // >= 1: the slot belongs to the row
    const float inv = 1.0f / (float)deg;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] * inv;
  }
  if constexpr (MODE == 2) {
    const int32_t *ap = arg + row * dim + c;
    const int4 alo = *reinterpret_cast<const int4 *>(ap), aup = *reinterpret_cast<const int4 *>(ap + 4);
    const int32_t w[8] = {alo.x, alo.y, alo.z, alo.w, aup.x, aup.y, aup.z, aup.w};
    const int32_t si = (int32_t)s;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w[j] == si ? v[j] : 0.f;
  }
  *reinterpret_cast<u32x4 *>(out + e * ld_out + c) = round8<DT>(v);
}

template <int DT>
void launch_spread(int mode, unsigned grid, hipStream_t st, const float *grad, int64_t ld_grad, const int32_t *arg,
                   const int32_t *rowptr, const int32_t *slot_row, const int32_t *perm, int64_t num_slots, int dim, int q,
                   int spb, uint16_t *out, int64_t ld_out) {
  if (mode == 0)
    k_segment_spread16<DT, 0><<<grid, 256, 0, st>>>(grad, ld_grad, arg, rowptr, slot_row, perm, num_slots, dim, q, spb, out, ld_out);
  else if (mode == 1)
    k_segment_spread16<DT, 1><<<grid, 256, 0, st>>>(grad, ld_grad, arg, rowptr, slot_row, perm, num_slots, dim, q, spb, out, ld_out);
  else
    k_segment_spread16<DT, 2><<<grid, 256, 0, st>>>(grad, ld_grad, arg, rowptr, slot_row, perm, num_slots, dim, q, spb, out, ld_out);
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_segment_reduce16_supported(int32_t msg_dim, int dtype) {
  return dtype_ok16(dtype) && shape_ok16(msg_dim) ? 1 : 0;
}

extern "C" int ptgnn_amd_segment_reduce16(const void *rows16, int64_t ld_rows, int dtype, const int32_t *rowptr,
                                          const int32_t *col, int64_t num_nodes, int32_t msg_dim, int reduce, float *out,
                                          int64_t ld_out, int32_t *argout, int64_t num_edges, int32_t hub_threshold,
                                          void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && msg_dim > 0 && num_edges >= 0, PTGNN_AMD_EINVAL, "segment_reduce16: bad sizes");
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "segment_reduce16: unknown reduce %d", reduce);
  PTGNN_REQUIRE(hub_threshold >= 0, PTGNN_AMD_EINVAL, "segment_reduce16: bad hub_threshold");
  PTGNN_REQUIRE(dtype_ok16(dtype), PTGNN_AMD_EINVAL,
                "segment_reduce16: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", dtype);
  PTGNN_REQUIRE(argout == nullptr || reduce >= PTGNN_AMD_MAX, PTGNN_AMD_EINVAL,
                "segment_reduce16: argout only with max/min");
  PTGNN_REQUIRE(shape_ok16(msg_dim), PTGNN_AMD_EUNSUPPORTED,
                "segment_reduce16: msg_dim=%d: needs msg_dim %% 32 == 0 and msg_dim <= 256", msg_dim);
  if (num_nodes == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && out && ld_out >= msg_dim, PTGNN_AMD_EINVAL, "segment_reduce16: null/ld");
  PTGNN_REQUIRE(rows16 || num_edges == 0, PTGNN_AMD_EINVAL, "segment_reduce16: null rows");
  PTGNN_REQUIRE(ld_rows >= msg_dim || num_edges == 0, PTGNN_AMD_EINVAL, "segment_reduce16: ld_rows=%lld < msg_dim=%d",
                (long long)ld_rows, msg_dim);
  PTGNN_REQUIRE(aligned16(rows16) && ld_rows % 8 == 0 && aligned16(out) && ld_out % 4 == 0 && aligned16(argout),
                PTGNN_AMD_EUNSUPPORTED,
                "segment_reduce16: rows, out and argout must be 16-byte aligned with ld_rows %% 8 == 0 and ld_out %% 4 == 0 "
                "(ld_rows=%lld, ld_out=%lld)", (long long)ld_rows, (long long)ld_out);
  SegArgs16 a{};
  a.rows = static_cast<const uint16_t *>(rows16); a.ld = ld_rows; a.rowptr = rowptr; a.col = col;
  a.msg_dim = msg_dim; a.num_nodes = num_nodes; a.out = out; a.ld_out = ld_out; a.argout = argout;
  a.hub_threshold = hub_threshold;
  hipStream_t st = (hipStream_t)stream_;
  if (dtype == PTGNN_AMD_HALF_BF16) launch_dtype<PTGNN_AMD_HALF_BF16>(a, reduce, st);
  else launch_dtype<PTGNN_AMD_HALF_F16>(a, reduce, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_SEGMENT_REDUCE16);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_segment_spread16_supported(int32_t dim, int dtype) {
  return dtype_ok16(dtype) && shape_ok16(dim) ? 1 : 0;
}

extern "C" int ptgnn_amd_segment_spread16(const float *grad, int64_t ld_grad, const int32_t *arg, const int32_t *rowptr,
                                          const int32_t *slot_row, const int32_t *perm, int64_t num_slots, int32_t dim,
                                          int reduce, int dtype, void *out16, int64_t ld_out, void *stream_) {
  PTGNN_REQUIRE(num_slots >= 0 && num_slots < ((int64_t)1 << 31) && dim > 0, PTGNN_AMD_EINVAL,
                "segment_spread16: bad sizes");
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "segment_spread16: unknown reduce %d", reduce);
  PTGNN_REQUIRE(dtype_ok16(dtype), PTGNN_AMD_EINVAL,
                "segment_spread16: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", dtype);
  PTGNN_REQUIRE(shape_ok16(dim), PTGNN_AMD_EUNSUPPORTED,
                "segment_spread16: dim=%d: needs dim %% 32 == 0 and dim <= 256", dim);
  if (num_slots == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(grad && slot_row && perm && out16, PTGNN_AMD_EINVAL, "segment_spread16: null pointer");
  PTGNN_REQUIRE(reduce < PTGNN_AMD_MAX || arg, PTGNN_AMD_EINVAL, "segment_spread16: max / min need the forward's arg");
  PTGNN_REQUIRE(reduce != PTGNN_AMD_MEAN || rowptr, PTGNN_AMD_EINVAL, "segment_spread16: mean needs rowptr");
  PTGNN_REQUIRE(ld_grad >= dim && ld_out >= dim, PTGNN_AMD_EINVAL, "segment_spread16: bad leading dimension");
  PTGNN_REQUIRE(aligned16(grad) && ld_grad % 4 == 0 && aligned16(out16) && ld_out % 8 == 0 && aligned16(arg),
                PTGNN_AMD_EUNSUPPORTED,
                "segment_spread16: grad, arg and out16 must be 16-byte aligned with ld_grad %% 4 == 0 and ld_out %% 8 == 0 "
                "(ld_grad=%lld, ld_out=%lld)", (long long)ld_grad, (long long)ld_out);
  const int q = dim / 8, spb = 256 / q;
  const unsigned grid = (unsigned)((num_slots + spb - 1) / spb);
  const int mode = reduce >= PTGNN_AMD_MAX ? 2 : (reduce == PTGNN_AMD_MEAN ? 1 : 0);
  hipStream_t st = (hipStream_t)stream_;
  uint16_t *out = static_cast<uint16_t *>(out16);
  if (dtype == PTGNN_AMD_HALF_BF16)
    launch_spread<PTGNN_AMD_HALF_BF16>(mode, grid, st, grad, ld_grad, arg, rowptr, slot_row, perm, num_slots, dim, q, spb, out, ld_out);
  else
    launch_spread<PTGNN_AMD_HALF_F16>(mode, grid, st, grad, ld_grad, arg, rowptr, slot_row, perm, num_slots, dim, q, spb, out, ld_out);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_SEGMENT_SPREAD16);
  return PTGNN_AMD_OK;
}
