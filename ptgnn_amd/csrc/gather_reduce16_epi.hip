// Segment reduce over 16-bit message rows with the MLP-MP layer's destination term and its GELU / LayerNorm finish (the
// opt-in half-width MLP-MP messages, ptgnn_amd/precision.py half_messages(mlp=True)):
//
//     out[v, :] = EPI( reduce over the CSR slots i of v of
//                      float(rows16[col[i] >> type_bits][t_i * M : + M]) + float(dst16[v][t_i * M : + M]) )
//
// t_i = col[i] & tmask; dst16 optional; rows bf16 or fp16; every addition, the fold, the mean, the GELU, the LayerNorm and
// the [N, M] output fp32; reduce = sum / mean / max / min; EPI = none, erf-GELU, affine LayerNorm, or GELU then LayerNorm.
// Contract + reference lines: include/ptgnn_amd.h (ptgnn_amd_gather_reduce16_epi).  The plain fold (no destination term,
// no finish) is gather_reduce16.hip and is untouched; a call without either is sent there by the host.
//
// Mapping: that of k_gather_reduce16 -- a lane owns 8 CONSECUTIVE columns (one 16-byte load per row), a destination row a
// group of LPR in {4, 8, 16, 32} lanes, slots fold in CSR order in groups of 8 with the next group's `col` entries
// requested behind the row loads, no atomics, hub rows folded by their whole workgroup in the same launch.  New here:
//   * DESTINATION TERM.  It depends on the slot's edge type, so it is added per slot BEFORE the fold (for max / min there
//     is no other place).  The lane's 16 bytes of dst16[v] for type t_i are a second load per slot, issued WITH the
//     group's row loads (8 + 8 loads in flight, 32 + 32 raw dwords), from a row all slots of v share: after the first
//     touch they are cache hits.  One IEEE addition per value and slot, then the fold: for max / min the bits of
//     max_i (fp32(a_i) + fp32(b_i)), for the sums the serial fp32 fold of those sums in CSR order.
//   * FINISH.  Mean rule, empty-row rule (max / min: 0), then the epilogue of the fp32 kernel (gather_reduce_core.h
//     RowOp::finish) in its order of operations: GELU per value; LayerNorm as mean = group sum / M, centred sum of
//     squares, 1 / sqrt(var + eps), (x - mean) * rstd * gamma + beta.  A row is spread over LPR lanes: both sums are
//     butterflies over the lane group (wave_ops.h group_sum<LPR>), lanes past M add 0 to them and store nothing.  The two
//     routes differ by the rounding of the rows (and by the association of the two row sums: 8 values per lane here).
//     An empty row still runs the epilogue: LayerNorm(0) is beta.
//   * HUB ROWS.  As in the plain kernel lane group q folds the q-th contiguous run of the row's slots -- the destination
//     term inside each run --, the partials meet in LDS and group 0 folds them in run order; group 0 then applies the mean
//     rule, the epilogue (all of its LPR lanes: the butterflies) and the store.
// The flags of the epilogue are a kernel argument (wave-uniform branches behind the edge loop), the destination term a
// template flag: it sits inside the loop.
#include <float.h>

#include "common.h"
#include "gather_reduce16.h"
#include "wave_ops.h"

namespace ptgnn_amd {
namespace {

struct ArgsEpi16 {
  const uint16_t *rows;      // 16-bit message rows, leading dimension ld (elements)
  int64_t ld;
  const uint16_t *dst;       // 16-bit destination-term rows [N, T * M], leading dimension ld_dst (HAS_DST only)
  int64_t ld_dst;
  const int32_t *rowptr;
  const int32_t *col;
  int32_t type_bits;
  int32_t msg_dim;
  int64_t row_begin, row_end;   // destination rows of this launch
  int64_t num_tiles;
  int32_t hub_threshold;     // rows with more in-edges are folded by their whole workgroup (0 = none)
  int32_t epi;               // PTGNN_AMD_EPI_*
  const float *ln_gamma, *ln_beta;
  float ln_eps;
  float *out;
  int64_t ld_out;
};

// One lane's share (8 columns from `colx`) of one destination row, or of one run of a hub row.
template <int DT, int LPR, int REDUCE, bool HAS_DST>
struct RowEpi16 {
  static constexpr bool kMinMax = REDUCE == PTGNN_AMD_MAX || REDUCE == PTGNN_AMD_MIN;
  static constexpr float kInit = REDUCE == PTGNN_AMD_MAX ? -FLT_MAX : (REDUCE == PTGNN_AMD_MIN ? FLT_MAX : 0.f);
  float acc[8];

  __device__ __forceinline__ RowEpi16() {
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

  // slots [beg, end) of destination row `row` in CSR order, groups of 8, one round trip per group
  __device__ __forceinline__ void reduce(const ArgsEpi16 &a, int colx, int64_t row, int beg, int end) {
    if (beg >= end) return;
    const int32_t tmask = (1 << a.type_bits) - 1;
    const int last = end - 1;
    const uint16_t *base = a.rows + colx;
    const uint16_t *dbase = HAS_DST ? a.dst + row * a.ld_dst + colx : nullptr;
    int32_t pk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pk[u] = a.col[beg + u < last ? beg + u : last];
    for (int i = beg; i < end; i += 8) {
      u32x4 raw[8], draw[HAS_DST ? 8 : 1];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t s = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        raw[u] = *reinterpret_cast<const u32x4 *>(base + s * a.ld + (int64_t)t * a.msg_dim);
        // the slot's destination term: the same row for every slot, so a cache hit after the first; in flight with the rows
        if constexpr (HAS_DST) draw[u] = *reinterpret_cast<const u32x4 *>(dbase + t * a.msg_dim);
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
        if constexpr (HAS_DST) {
          float b[8];
#pragma unroll
          for (int d = 0; d < 4; ++d) widen2<DT>(draw[u][d], b[2 * d], b[2 * d + 1]);
#pragma unroll
          for (int v = 0; v < 8; ++v) m[v] += b[v];                 // one IEEE addition per slot, before the fold
        }
        if (!kMinMax) {
#pragma unroll
          for (int v = 0; v < 8; ++v) m[v] = valid ? m[v] : 0.f;   // a clamped duplicate adds nothing
        }
        fold(m);                                                    // max / min: a duplicate never beats itself
      }
    }
  }

  // Mean / empty-segment rule, then the epilogue; EVERY lane of the row's lane group calls it (the LayerNorm sums are
  // butterflies over the group).  `active`: this lane's 8 columns are inside M.
  __device__ __forceinline__ void finish(const ArgsEpi16 &a, int colx, bool active, int deg) {
    if (REDUCE == PTGNN_AMD_MEAN) {
      const float cnt = (float)(deg < 1 ? 1 : deg);
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = acc[v] / cnt;
    }
    if (kMinMax && deg == 0) {
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = 0.f;                    // torch_scatter: empty segment -> 0
    }
    if (a.epi & PTGNN_AMD_EPI_GELU) {
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = gelu_erf(acc[v]);
    }
    if (a.epi & PTGNN_AMD_EPI_LAYERNORM) {
      const float fm = (float)a.msg_dim;
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < 8; ++v) s += active ? acc[v] : 0.f;      // lanes past M contribute nothing
      const float mean = group_sum<LPR>(s) / fm;
      float q = 0.f;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const float dlt = acc[v] - mean;
        q += active ? dlt * dlt : 0.f;
      }
      const float rstd = 1.0f / sqrtf(group_sum<LPR>(q) / fm + a.ln_eps);
      if (active) {
        const float4 g0 = *reinterpret_cast<const float4 *>(a.ln_gamma + colx);
        const float4 g1 = *reinterpret_cast<const float4 *>(a.ln_gamma + colx + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(a.ln_beta + colx);
        const float4 b1 = *reinterpret_cast<const float4 *>(a.ln_beta + colx + 4);
        const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v] = (acc[v] - mean) * rstd * gm[v] + bt[v];
      }
    }
  }

  // the row's 8 columns as two float4
  __device__ __forceinline__ void store(float *orow) const {
    *reinterpret_cast<float4 *>(orow) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4 *>(orow + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
};

template <int DT, int LPR, int REDUCE, bool HAS_DST>
__device__ __forceinline__ void gather_reduce16_epi_body(const ArgsEpi16 &a) {
  using Op = RowEpi16<DT, LPR, REDUCE, HAS_DST>;
  constexpr int G = 256 / LPR;           // destination rows (lane groups) per workgroup
  constexpr int W = LPR * 8;             // columns a lane group spans (>= msg_dim)
  __shared__ __attribute__((aligned(16))) float part[G * W];
  __shared__ int long_flag[G];

  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;       // whole workgroup: before any barrier
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int colx = g * 8;
  const bool active = colx < a.msg_dim;  // lanes past M load and store nothing, but stay for their group's butterflies
  const int64_t row0 = a.row_begin + tile * G;
  const int64_t row = row0 + grp;

  int beg = 0, end = 0;
  if (row < a.row_end) {
    beg = a.rowptr[row];
    end = a.rowptr[row + 1];
  }
  const bool is_long = a.hub_threshold > 0 && end - beg > a.hub_threshold;
  if (row < a.row_end && !is_long) {     // uniform over the lane group
    Op op;
    if (active) op.reduce(a, colx, row, beg, end);
    op.finish(a, colx, active, end - beg);
    if (active) op.store(a.out + row * a.ld_out + colx);
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
    Op op;
    if (active) op.reduce(a, colx, r, b, e);         // the destination term of row r inside every run
    if (grp != 0 && active) {
#pragma unroll
      for (int v = 0; v < 8; ++v) part[grp * W + colx + v] = op.acc[v];
    }
    __syncthreads();
    if (grp == 0) {
      if (active) {
        for (int p = 1; p < G; ++p) {    // fixed combine order => deterministic
          float m[8];
          const float4 lo = *reinterpret_cast<const float4 *>(part + p * W + colx);
          const float4 hi = *reinterpret_cast<const float4 *>(part + p * W + colx + 4);
          m[0] = lo.x; m[1] = lo.y; m[2] = lo.z; m[3] = lo.w;
          m[4] = hi.x; m[5] = hi.y; m[6] = hi.z; m[7] = hi.w;
          op.fold(m);                     // an empty run holds the initial value: it changes nothing
        }
      }
      op.finish(a, colx, active, rend - rbeg);       // all LPR lanes of group 0
      if (active) op.store(a.out + r * a.ld_out + colx);
    }
    __syncthreads();                      // group 0 is done with `part` before the next long row fills it
  }
}

// Two kernels over the one body, for the register budget alone.  Without a destination term the body fits the 96 VGPRs
// of 5 waves per SIMD -- the best the plain kernel reaches (its bf16 sum) -- once the compiler is asked for them; with it
// (32 more raw dwords in flight) that request spills, so that kernel is left at the compiler's 115 - 116 VGPRs: 4 waves,
// the plain kernel's occupancy everywhere but its bf16 sum.  No scratch in either.
template <int DT, int LPR, int REDUCE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_gather_reduce16_epi(ArgsEpi16 a) {
  gather_reduce16_epi_body<DT, LPR, REDUCE, false>(a);
}

template <int DT, int LPR, int REDUCE>
__global__ __launch_bounds__(256) void k_gather_reduce16_dst_epi(ArgsEpi16 a) {
  gather_reduce16_epi_body<DT, LPR, REDUCE, true>(a);
}

template <int DT, int LPR, int REDUCE, bool HAS_DST>
void launch_kernel(const ArgsEpi16 &a, unsigned grid, hipStream_t st) {
  if constexpr (HAS_DST) k_gather_reduce16_dst_epi<DT, LPR, REDUCE><<<grid, 256, 0, st>>>(a);
  else k_gather_reduce16_epi<DT, LPR, REDUCE><<<grid, 256, 0, st>>>(a);
}

template <int DT, int LPR, bool HAS_DST>
void launch_reduce(const ArgsEpi16 &a0, int reduce, hipStream_t st) {
  ArgsEpi16 a = a0;
  constexpr int G = 256 / LPR;
  a.num_tiles = (a.row_end - a.row_begin + G - 1) / G;
  const unsigned grid = (unsigned)xcd_padded_blocks(a.num_tiles);
  switch (reduce) {
    case PTGNN_AMD_SUM: launch_kernel<DT, LPR, PTGNN_AMD_SUM, HAS_DST>(a, grid, st); break;
    case PTGNN_AMD_MEAN: launch_kernel<DT, LPR, PTGNN_AMD_MEAN, HAS_DST>(a, grid, st); break;
    case PTGNN_AMD_MAX: launch_kernel<DT, LPR, PTGNN_AMD_MAX, HAS_DST>(a, grid, st); break;
    default: launch_kernel<DT, LPR, PTGNN_AMD_MIN, HAS_DST>(a, grid, st); break;
  }
}

template <int DT, bool HAS_DST>
void launch_lanes(const ArgsEpi16 &a, int reduce, hipStream_t st) {
  const int lanes = a.msg_dim / 8;
  if (lanes <= 4) launch_reduce<DT, 4, HAS_DST>(a, reduce, st);
  else if (lanes <= 8) launch_reduce<DT, 8, HAS_DST>(a, reduce, st);
  else if (lanes <= 16) launch_reduce<DT, 16, HAS_DST>(a, reduce, st);
  else launch_reduce<DT, 32, HAS_DST>(a, reduce, st);
}

template <int DT>
void launch_dtype(const ArgsEpi16 &a, int reduce, hipStream_t st) {
  if (a.dst) launch_lanes<DT, true>(a, reduce, st);
  else launch_lanes<DT, false>(a, reduce, st);
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_gather_reduce16_epi(const void *rows16, int64_t ld_rows, const void *dst16, int64_t ld_dst,
                                             int dtype, const int32_t *rowptr, const int32_t *col, int32_t type_bits,
                                             int64_t num_nodes, int32_t msg_dim, int reduce, int epilogue,
                                             const float *ln_gamma, const float *ln_beta, float ln_eps, float *out,
                                             int64_t ld_out, int64_t num_edges, int32_t hub_threshold, int64_t row_begin,
                                             int64_t row_end, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && msg_dim > 0 && num_edges >= 0, PTGNN_AMD_EINVAL, "gather_reduce16_epi: bad sizes");
  PTGNN_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= num_nodes, PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: row range [%lld, %lld) outside [0, %lld]", (long long)row_begin,
                (long long)row_end, (long long)num_nodes);
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: unknown reduce %d", reduce);
  PTGNN_REQUIRE(epilogue >= 0 && epilogue <= PTGNN_AMD_EPI_GELU_LAYERNORM, PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: bad epilogue %d", epilogue);
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "gather_reduce16_epi: bad type_bits");
  PTGNN_REQUIRE(hub_threshold >= 0, PTGNN_AMD_EINVAL, "gather_reduce16_epi: bad hub_threshold");
  PTGNN_REQUIRE(dtype_ok16(dtype), PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", dtype);
  PTGNN_REQUIRE(shape_ok16(msg_dim), PTGNN_AMD_EUNSUPPORTED,
                "gather_reduce16_epi: msg_dim=%d: needs msg_dim %% 32 == 0 and msg_dim <= 256", msg_dim);
  const bool ln = (epilogue & PTGNN_AMD_EPI_LAYERNORM) != 0;
  PTGNN_REQUIRE(!ln || (ln_gamma && ln_beta), PTGNN_AMD_EINVAL, "gather_reduce16_epi: LayerNorm epilogue needs gamma/beta");
  if (row_begin == row_end) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && out && ld_out >= msg_dim, PTGNN_AMD_EINVAL, "gather_reduce16_epi: null/ld");
  // a plan without edges reads no message row and no destination term: both tables may be null pointers
  PTGNN_REQUIRE(rows16 || num_edges == 0, PTGNN_AMD_EINVAL, "gather_reduce16_epi: null rows");
  PTGNN_REQUIRE(ld_rows >= msg_dim || num_edges == 0, PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: ld_rows=%lld < msg_dim=%d", (long long)ld_rows, msg_dim);
  PTGNN_REQUIRE(!dst16 || ld_dst >= msg_dim || num_edges == 0, PTGNN_AMD_EINVAL,
                "gather_reduce16_epi: ld_dst=%lld < msg_dim=%d", (long long)ld_dst, msg_dim);
  PTGNN_REQUIRE(aligned16(rows16) && ld_rows % 8 == 0 && aligned16(out) && ld_out % 4 == 0 &&
                    (!dst16 || (aligned16(dst16) && ld_dst % 8 == 0)) &&
                    (!ln || (aligned16(ln_gamma) && aligned16(ln_beta))),
                PTGNN_AMD_EUNSUPPORTED,
                "gather_reduce16_epi: rows, dst, out, gamma and beta must be 16-byte aligned with ld_rows %% 8 == 0, "
                "ld_dst %% 8 == 0 and ld_out %% 4 == 0 (ld_rows=%lld, ld_dst=%lld, ld_out=%lld)", (long long)ld_rows,
                (long long)ld_dst, (long long)ld_out);
  ArgsEpi16 a{};
  a.rows = static_cast<const uint16_t *>(rows16); a.ld = ld_rows;
  a.dst = num_edges > 0 ? static_cast<const uint16_t *>(dst16) : nullptr; a.ld_dst = ld_dst;
  a.rowptr = rowptr; a.col = col; a.type_bits = type_bits; a.msg_dim = msg_dim; a.row_begin = row_begin;
  a.row_end = row_end; a.out = out; a.ld_out = ld_out; a.hub_threshold = hub_threshold;
  a.epi = epilogue; a.ln_gamma = ln_gamma; a.ln_beta = ln_beta; a.ln_eps = ln_eps;
  hipStream_t st = (hipStream_t)stream_;
  if (dtype == PTGNN_AMD_HALF_BF16) launch_dtype<PTGNN_AMD_HALF_BF16>(a, reduce, st);
  else launch_dtype<PTGNN_AMD_HALF_F16>(a, reduce, st);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_AGG16_EPI);
  return PTGNN_AMD_OK;
}
