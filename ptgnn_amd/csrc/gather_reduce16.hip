// Segment reduce over 16-bit message rows (the opt-in half-width GGNN messages, ptgnn_amd/precision.py half_messages):
//
//     out[v, :] = reduce over the CSR slots i of v of float(rows16[col[i] >> type_bits][(col[i] & tmask) * M : + M])
//
// rows bf16 or fp16, accumulation and the [N, M] output fp32, reduce = sum / mean / max / min.
// Contract + reference lines: include/ptgnn_amd.h (ptgnn_amd_gather_reduce16).  The fp32 walk is gather_reduce_core.h
// and is untouched; this file shares nothing with it but the tile order (xcd_swizzle) and the caller's hub threshold.
//
// Mapping (HBM / L2-bound like the fp32 walk, at half its bytes per edge: 2 M + 4):
//   * a lane owns 8 CONSECUTIVE columns, so one 16-byte load carries 8 values -- the 16 B / lane coalescing of the fp32
//     walk (a float4-shaped walk over 16-bit rows would ask for 8 B / lane);
//   * a destination row belongs to a group of LPR lanes, LPR = the power of two >= M / 8 in {4, 8, 16, 32}: a wave folds
//     64 / LPR rows, a 256-thread workgroup 256 / LPR; lanes past M are idle (they load and store nothing);
//   * the values become fp32 in registers: a bf16 pair is a shift and a mask of its dword, an fp16 pair one convert of
//     the packed pair; a lane holds 8 fp32 accumulators, slots fold in CSR order, no atomics;
//   * the edge loop runs in groups of 8 slots: all 8 row loads (128 B per lane) are issued before the first is used and
//     the next group's `col` entries are requested behind them.  A short row or a tail is one more group with its indices
//     clamped to the row's last slot: the duplicates are zeroed for the sums and change nothing in a strict max / min;
//   * rows up to `hub_threshold` in-edges -- the rows beyond kLongRow included -- fold serially on their lane group, in
//     CSR order: the bits of the serial fp32 fold of the up-cast values, as the fp32 walk gives for them;
//   * HUB rows (more than `hub_threshold` in-edges; this walk reads no hub list, takes no tickets and needs no side
//     stream) are left out of the lane groups' pass and folded by their WHOLE workgroup afterwards: lane group q takes
//     the q-th contiguous run of the row's slots, the partials meet in LDS and group 0 folds them in run order.  One
//     launch, fixed order: deterministic, and for max / min the earliest slot still wins a tie of zeros.  The fold
//     ORDER of a hub row's sum differs from the serial order (fp32 rounding only), as the fp32 hub rows' does.
// No destination term, no arg output, no epilogue, no mask here: the destination term and the GELU / LayerNorm finish
// of the MLP-MP layer are gather_reduce16_epi.hip (same mapping); arg and mask stay on the fp32 rows.
#include <float.h>

#include "common.h"
#include "gather_reduce16.h"

namespace ptgnn_amd {
namespace {

struct Args16 {
  const uint16_t *rows;      // 16-bit message rows, leading dimension ld (elements)
  int64_t ld;
  const int32_t *rowptr;
  const int32_t *col;
  int32_t type_bits;
  int32_t msg_dim;
  int64_t row_begin, row_end;   // destination rows of this launch
  int64_t num_tiles;
  int32_t hub_threshold;     // rows with more in-edges are folded by their whole workgroup (0 = none)
  float *out;
  int64_t ld_out;
};

// One lane's share (8 columns from `colx`) of one destination row, or of one run of a hub row.
template <int DT, int REDUCE>
struct Row16 {
  static constexpr bool kMinMax = REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN;
  static constexpr float kInit = REDUCE == PTGNN_AMD_MAX ? -FLT_MAX : (REDUCE == PTGNN_AMD_MIN ? FLT_MAX : 0.f);
  float acc[8];

  __device__ __forceinline__ Row16() {
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = kInit;
  }

  __device__ __forceinline__ void fold(const float (&m)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      if (REDUCE == PTGNN_AMD_MAX) acc[v] = m[v] > acc[v] ? m[v] : acc[v];        // strict: the earlier slot stays
      else if (REDUCE == PTGNN_AMD_MIN) acc[v] = m[v] < acc[v] ? m[v] : acc[v];
      else acc[v] += m[v];
    }
  }

  // slots [beg, end) in CSR order, groups of 8, one round trip per group
  __device__ __forceinline__ void reduce(const Args16 &a, int colx, int beg, int end) {
    if (beg >= end) return;
    const int32_t tmask = (1 << a.type_bits) - 1;
    const int last = end - 1;
    const uint16_t *base = a.rows + colx;
    int32_t pk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pk[u] = a.col[beg + u < last ? beg + u : last];
    for (int i = beg; i < end; i += 8) {
      u32x4 raw[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t s = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        raw[u] = *reinterpret_cast<const u32x4 *>(base + s * a.ld + (int64_t)t * a.msg_dim);
      }
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
        if (!kMinMax) {
#pragma unroll
          for (int v = 0; v < 8; ++v) m[v] = valid ? m[v] : 0.f;   // a clamped duplicate adds nothing
        }
        fold(m);                                                    // max / min: a duplicate never beats itself
      }
    }
  }

  // mean / empty-segment rule, then the row's 8 columns as two float4
  __device__ __forceinline__ void finish_and_store(float *orow, int deg) {
    if (REDUCE == PTGNN_AMD_MEAN) {
      const float cnt = (float)(deg < 1 ? 1 : deg);
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = acc[v] / cnt;
    }
    if (kMinMax && deg == 0) {
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = 0.f;                    // torch_scatter: empty segment -> 0
    }
    *reinterpret_cast<float4 *>(orow) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4 *>(orow + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
};

template <int DT, int LPR, int REDUCE>
__global__ __launch_bounds__(256) void k_gather_reduce16(Args16 a) {
  constexpr int G = 256 / LPR;           // destination rows (lane groups) per workgroup
  constexpr int W = LPR * 8;             // columns a lane group spans (>= msg_dim)
  __shared__ __attribute__((aligned(16))) float part[G * W];
  __shared__ int long_flag[G];

  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;       // whole workgroup: before any barrier
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int colx = g * 8;
  const bool active = colx < a.msg_dim;  // lanes past M are idle
  const int64_t row0 = a.row_begin + tile * G;
  const int64_t row = row0 + grp;

  int beg = 0, end = 0;
  if (row < a.row_end) {
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
  }
  const bool is_long = a.hub_threshold > 0 && end - beg > a.hub_threshold;
  if (row < a.row_end && !is_long && active) {
    Row16<DT, REDUCE> op;
    op.reduce(a, colx, beg, end);
    op.finish_and_store(a.out + row * a.ld_out + colx, end - beg);
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
    Row16<DT, REDUCE> op;
    if (active) op.reduce(a, colx, b, e);
    if (grp != 0) {
#pragma unroll
      for (int v = 0; v < 8; ++v) part[grp * W + colx + v] = op.acc[v];
    }
    __syncthreads();
    if (grp == 0 && active) {
      for (int p = 1; p < G; ++p) {      // fixed combine order => deterministic
        float m[8];
        const float4 lo = *reinterpret_cast<const float4 *>(part + p * W + colx);
        const float4 hi = *reinterpret_cast<const float4 *>(part + p * W + colx + 4);
        m[0] = lo.x; m[1] = lo.y; m[2] = lo.z; m[3] = lo.w;
        m[4] = hi.x; m[5] = hi.y; m[6] = hi.z; m[7] = hi.w;
        op.fold(m);                       // an empty run holds the initial value: it changes nothing
      }
      op.finish_and_store(a.out + r * a.ld_out + colx, rend - rbeg);
    }
    __syncthreads();                      // group 0 is done with `part` before the next long row fills it
  }
}

template <int DT, int LPR>
void launch_reduce(const Args16 &a0, int reduce, hipStream_t st) {
  Args16 a = a0;
  constexpr int G = 256 / LPR;
  a.num_tiles = (a.row_end - a.row_begin + G - 1) / G;
  const unsigned grid = (unsigned)xcd_padded_blocks(a.num_tiles);
  switch (reduce) {
    case PTGNN_AMD_SUM: k_gather_reduce16<DT, LPR, PTGNN_AMD_SUM><<<grid, 256, 0, st>>>(a); break;
    case PTGNN_AMD_MEAN: k_gather_reduce16<DT, LPR, PTGNN_AMD_MEAN><<<grid, 256, 0, st>>>(a); break;
    case PTGNN_AMD_MAX: k_gather_reduce16<DT, LPR, PTGNN_AMD_MAX><<<grid, 256, 0, st>>>(a); break;
    default: k_gather_reduce16<DT, LPR, PTGNN_AMD_MIN><<<grid, 256, 0, st>>>(a); break;
  }
}

template <int DT>
void launch_dtype(const Args16 &a, int reduce, hipStream_t st) {
  const int lanes = a.msg_dim / 8;
  if (lanes <= 4) launch_reduce<DT, 4>(a, reduce, st);
  else if (lanes <= 8) launch_reduce<DT, 8>(a, reduce, st);
  else if (lanes <= 16) launch_reduce<DT, 16>(a, reduce, st);
  else launch_reduce<DT, 32>(a, reduce, st);
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_gather_reduce16_supported(int32_t msg_dim, int dtype) {
  return dtype_ok16(dtype) && shape_ok16(msg_dim) ? 1 : 0;
}

extern "C" int ptgnn_amd_gather_reduce16(const void *rows16, int64_t ld_rows, int dtype, const int32_t *rowptr,
                                         const int32_t *col, int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                         int reduce, float *out, int64_t ld_out, int64_t num_edges,
                                         int32_t hub_threshold, int64_t row_begin, int64_t row_end, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && msg_dim > 0 && num_edges >= 0, PTGNN_AMD_EINVAL, "gather_reduce16: bad sizes");
  PTGNN_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= num_nodes, PTGNN_AMD_EINVAL,
                "gather_reduce16: row range [%lld, %lld) outside [0, %lld]", (long long)row_begin, (long long)row_end,
                (long long)num_nodes);
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "gather_reduce16: unknown reduce %d", reduce);
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "gather_reduce16: bad type_bits");
  PTGNN_REQUIRE(hub_threshold >= 0, PTGNN_AMD_EINVAL, "gather_reduce16: bad hub_threshold");
  PTGNN_REQUIRE(dtype_ok16(dtype), PTGNN_AMD_EINVAL, "gather_reduce16: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16",
                dtype);
  PTGNN_REQUIRE(shape_ok16(msg_dim), PTGNN_AMD_EUNSUPPORTED,
                "gather_reduce16: msg_dim=%d: needs msg_dim %% 32 == 0 and msg_dim <= 256", msg_dim);
  if (row_begin == row_end) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && out && ld_out >= msg_dim, PTGNN_AMD_EINVAL, "gather_reduce16: null/ld");
  // a plan without edges reads no message row: its table may be a null pointer
  PTGNN_REQUIRE(rows16 || num_edges == 0, PTGNN_AMD_EINVAL, "gather_reduce16: null rows");
  PTGNN_REQUIRE(ld_rows >= msg_dim || num_edges == 0, PTGNN_AMD_EINVAL, "gather_reduce16: ld_rows=%lld < msg_dim=%d",
                (long long)ld_rows, msg_dim);
  PTGNN_REQUIRE(aligned16(rows16) && ld_rows % 8 == 0 && aligned16(out) && ld_out % 4 == 0, PTGNN_AMD_EUNSUPPORTED,
                "gather_reduce16: rows and out must be 16-byte aligned with ld_rows %% 8 == 0 and ld_out %% 4 == 0 "
                "(ld_rows=%lld, ld_out=%lld)", (long long)ld_rows, (long long)ld_out);
  Args16 a{};
  a.rows = static_cast<const uint16_t *>(rows16); a.ld = ld_rows; a.rowptr = rowptr; a.col = col;
  a.type_bits = type_bits; a.msg_dim = msg_dim; a.row_begin = row_begin; a.row_end = row_end;
  a.out = out; a.ld_out = ld_out; a.hub_threshold = hub_threshold;
  hipStream_t st = (hipStream_t)stream_;
  if (dtype == PTGNN_AMD_HALF_BF16) launch_dtype<PTGNN_AMD_HALF_BF16>(a, reduce, st);
  else launch_dtype<PTGNN_AMD_HALF_F16>(a, reduce, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_AGG16);
  return PTGNN_AMD_OK;
}
