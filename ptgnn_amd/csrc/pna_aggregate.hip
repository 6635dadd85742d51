// PNA aggregation (pna_aggregation.py:27-56), forward and backward, over the CSR plan of ptgnn_amd_csr_build.
// Contract: include/ptgnn_amd.h (ptgnn_amd_pna_aggregate_f32 / _backward_f32).
//
// Per destination row v with in-degree d and message rows m_e (e in the row's CSR slots, message order):
//     A    = [sum, mean, max, min, std]                               (5 blocks of M columns)
//     sum  = sum_e m_e                          mean = sum / (float(d) + 1e-5)
//     max / min: torch_scatter (0 for an empty row; on ties the earliest slot is the arg)
//     std  = sqrt(sum_e (relu(m_e*m_e - mean*mean) + 1e-10))
//     s    = log(float(d) + 1) / delta          s' = 1 / (s + 1e-3)
//     out  = [A | A*s | A*s']                                         (15 blocks of M columns)
// optionally followed by GELU and an affine LayerNorm over the 15M columns (the MLP layer's message activation and
// first state-update block), so inference never writes the pre-LayerNorm row.
//
// Mapping (HBM-bound; the lane-group row walk of RowOp in gather_reduce_core.h, restated in PnaRow below):
//   * rows with d <= kPnaLong: one row per group of LPR lanes, each lane owning VEC-wide column chunks; pass 1 folds
//     sum / max / min (+ arg) in slot order over prefetched groups of U slots (the next group's `col` entries ride
//     behind the current group's rows), pass 2 re-walks the same slots for the std sum -- the rows were just read,
//     so the second pass is L2 traffic -- and the finish writes the 15M-wide row;
//   * rows with d > kPnaLong (power-law hubs): a second launch gives each such row a WORKGROUP.  Its lane groups
//     take the row's slots interleaved, the partials (sum / max / min / arg, then the std sums) combine in LDS in
//     lane-group order, so results are deterministic run to run (the sum's rounding order differs from the serial
//     fold; max / min and their arg are exact).  One launch does both passes: the mean between them is a workgroup
//     barrier, where the chunk / ticket hub machinery of gather_reduce_core.h would need two grid-wide phases.
//   * messages: the table form (ysrc[src, t*M..] + optional destination term ydst[v, t*M..], `col` packs src and
//     type) or the edge form ([E, M] messages, col = plan.perm, type_bits = 0).
// Arithmetic: fp32, IEEE division and sqrt, no contraction (m*m and mean*mean round before the subtraction, as the
// reference's pow / sub do), so degree-1 rows -- where m*m - mean*mean is ~2e-5 m*m -- keep the reference's bits.
// Algorithmic bytes (forward): per edge 4*M (message row) + 4 (col); per node 4 (rowptr) + 60*M (out)
//   [+ 4*M destination term] [+ 8*M argmax / argmin].
#include <hip/hip_fp16.h>

#include "gather_reduce_core.h"   // xcd_swizzle, group_sum, gelu_erf, IC

#pragma clang fp contract(off)

namespace ptgnn_amd {
namespace {

constexpr int kPnaLong = 256;   // rows with more in-edges take the workgroup-per-row launch

struct PnaArgs {
  const float *ysrc;
  const float *ydst;
  int64_t ld_y, ld_yd;
  const int32_t *rowptr;
  const int32_t *col;
  int32_t type_bits;
  int64_t num_nodes;
  int32_t msg_dim;
  float delta;
  int32_t epi;
  const float *ln_gamma, *ln_beta;
  float ln_eps;
  int32_t round_mode;        // A rounded to this message dtype before the scalers: 0 none, 1 fp16, 2 bf16
  float *out;
  int64_t ld_out;
  int32_t *argmax, *argmin;  // [N, M] winning CSR slot (-1: empty row)
  float *agg_out;            // nullable [N, 5M]: A before the rounding to the message dtype (the backward's input)
  int64_t num_tiles;
  // backward
  const float *agg;          // the forward's A (mean at column M, std at 4M), leading dimension ld_agg
  int64_t ld_agg;
  const int32_t *amax, *amin;
  const float *grad;         // dL/dout [N, 15M]
  int64_t ld_grad;
  float *gmsg;               // [E, M] in message order: row col[slot]
  int64_t ld_gmsg;
};

__device__ __forceinline__ float round_to(float x, int mode) {
  if (mode == 1) return __half2float(__float2half_rn(x));
  if (mode == 2) {   // bfloat16, round to nearest even (finite values; NaN stays NaN)
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return x;
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    return __uint_as_float(u);
  }
  return x;
}

// DST: 0 no destination term, 1 one per slot (several edge types), 2 one per row (one edge type: loaded once)
// EPI: the GELU / LayerNorm finish is compiled in (its 15M-wide row stays in registers: ~150 VGPRs against ~80)
template <int VEC, int LPR, int CH, int DST, bool HAS_ARG, bool EPI = false>
struct PnaRow {
  static constexpr int W = LPR * VEC * CH;   // columns of one column block
  const PnaArgs &a;
  const int g, cbase, M;
  const int32_t tmask;
  float sum[CH][VEC], mx[CH][VEC], mn[CH][VEC], sq[CH][VEC], mean[CH][VEC];
  int amx[CH][VEC], amn[CH][VEC];

  __device__ __forceinline__ PnaRow(const PnaArgs &a_, int g_, int cbase_)
      : a(a_), g(g_), cbase(cbase_), M(a_.msg_dim), tmask((1 << a_.type_bits) - 1) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        sum[c][v] = 0.f; sq[c][v] = 0.f; mean[c][v] = 0.f;
        mx[c][v] = -INFINITY; mn[c][v] = INFINITY;
        amx[c][v] = -1; amn[c][v] = -1;
      }
  }

  __device__ __forceinline__ int colx(int c) const { return cbase + (g + c * LPR) * VEC; }

  __device__ __forceinline__ void load_row(const float *base, float (&dst)[CH][VEC]) const {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int x = colx(c);
      if constexpr (VEC == 4) {
        if (x < M) {
          const float4 t = *reinterpret_cast<const float4 *>(base + x);
          dst[c][0] = t.x; dst[c][1] = t.y; dst[c][2] = t.z; dst[c][3] = t.w;
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) dst[c][v] = 0.f;
        }
      } else {
        dst[c][0] = x < M ? base[x] : 0.f;
      }
    }
  }

  // Slots beg, beg+stride, ... < end of row `row` in groups of U, one round trip per group: f(m, slot, valid, msg_row)
  // per slot in order.  A short group is padded with the row's last slot (valid = false).
  template <int U, typename F>
  __device__ __forceinline__ void walk(int64_t row, int beg, int end, int stride, F &&f) const {
    if (beg >= end) return;
    const float *dst_base = DST ? a.ydst + row * a.ld_yd : nullptr;
    const int last = beg + ((end - 1 - beg) / stride) * stride;
    float d1[CH][VEC];
    if constexpr (DST == 2) load_row(dst_base, d1);
    int32_t pk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = beg + u * stride;
      pk[u] = a.col[idx < last ? idx : last];
    }
    for (int i = beg; i < end; i += U * stride) {
      float m[U][CH][VEC];
      float d[DST == 1 ? U : 1][CH][VEC];
      int32_t src[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        src[u] = pk[u] >> a.type_bits;
        const int t = pk[u] & tmask;
        load_row(a.ysrc + src[u] * a.ld_y + (int64_t)t * M, m[u]);
        if constexpr (DST == 1) load_row(dst_base + (int64_t)t * M, d[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = i + (U + u) * stride;
        pk[u] = a.col[idx < last ? idx : last];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = i + u * stride;
        const bool valid = idx < end;
        if constexpr (DST != 0) {
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) m[u][c][v] += DST == 2 ? d1[c][v] : d[DST == 1 ? u : 0][c][v];
        }
        f(m[u], valid ? idx : last, valid, src[u]);
      }
    }
  }

  static constexpr int kU = DST == 1 ? 4 : 8;   // a per-slot destination term doubles the rows in flight

  // pass 1: sum / max / min (+ arg) in slot order; on ties the earlier slot stays (strict compares)
  __device__ __forceinline__ void pass1(int64_t row, int beg, int end, int stride) {
    walk<kU>(row, beg, end, stride, [&](const float (&m)[CH][VEC], int slot, bool valid, int64_t) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          sum[c][v] += valid ? m[c][v] : 0.f;
          if (m[c][v] > mx[c][v]) { mx[c][v] = m[c][v]; if (HAS_ARG) amx[c][v] = slot; }
          if (m[c][v] < mn[c][v]) { mn[c][v] = m[c][v]; if (HAS_ARG) amn[c][v] = slot; }
        }
    });
  }

  __device__ __forceinline__ void set_mean(int deg) {
    const float den = (float)deg + 1e-5f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) mean[c][v] = sum[c][v] / den;
  }

  // pass 2: sum_e relu(m*m - mean*mean) + 1e-10 in slot order
  __device__ __forceinline__ void pass2(int64_t row, int beg, int end, int stride) {
    float mm[CH][VEC];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) mm[c][v] = mean[c][v] * mean[c][v];
    walk<kU>(row, beg, end, stride, [&](const float (&m)[CH][VEC], int, bool valid, int64_t) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float q = m[c][v] * m[c][v] - mm[c][v];
          const float comp = (q > 0.f ? q : 0.f) + 1e-10f;
          sq[c][v] += valid ? comp : 0.f;
        }
    });
  }

  // fold another lane group's pass-1 partial (slots interleaved with ours): ties -> the lower slot
  __device__ __forceinline__ void combine1(const float (&s)[CH][VEC], const float (&x)[CH][VEC], const int (&ax)[CH][VEC],
                                           const float (&n)[CH][VEC], const int (&an)[CH][VEC]) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        sum[c][v] += s[c][v];
        bool take = x[c][v] > mx[c][v];
        if (HAS_ARG) take = take || (x[c][v] == mx[c][v] && ax[c][v] >= 0 && (amx[c][v] < 0 || ax[c][v] < amx[c][v]));
        if (take) { mx[c][v] = x[c][v]; if (HAS_ARG) amx[c][v] = ax[c][v]; }
        take = n[c][v] < mn[c][v];
        if (HAS_ARG) take = take || (n[c][v] == mn[c][v] && an[c][v] >= 0 && (amn[c][v] < 0 || an[c][v] < amn[c][v]));
        if (take) { mn[c][v] = n[c][v]; if (HAS_ARG) amn[c][v] = an[c][v]; }
      }
  }

  // A, the scalers, the optional GELU + LayerNorm, and the stores of the 15M-wide row (+ args)
  __device__ __forceinline__ void finish_and_store(int64_t row, int deg) {
    const float dd = (float)deg;
    float A[5][CH][VEC];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        A[0][c][v] = sum[c][v];
        A[1][c][v] = mean[c][v];
        A[2][c][v] = deg > 0 ? mx[c][v] : 0.f;   // torch_scatter: an empty segment is 0
        A[3][c][v] = deg > 0 ? mn[c][v] : 0.f;
        A[4][c][v] = sqrtf(sq[c][v]);
      }
    if (a.agg_out) {
#pragma unroll
      for (int k = 0; k < 5; ++k) store(a.agg_out + row * (int64_t)(5 * M) + k * M, A[k]);
    }
    if (a.round_mode) {
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) A[k][c][v] = round_to(A[k][c][v], a.round_mode);
    }
    const float s1 = logf(dd + 1.0f) / a.delta;
    const float s2 = 1.0f / (s1 + 1e-3f);
    float *orow = a.out + row * a.ld_out;
    if (!EPI || a.epi == 0) {
#pragma unroll
      for (int k = 0; k < 15; ++k) {
        const float sc = k < 5 ? 1.f : (k < 10 ? s1 : s2);
        float o[CH][VEC];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) o[c][v] = k < 5 ? A[k][c][v] : A[k % 5][c][v] * sc;
        store(orow + k * M, o);
      }
    } else {
      // the whole 15M-wide row lives in this lane group (one column block, cbase == 0: host checks)
      float y[15][CH][VEC];
      float part = 0.f;
#pragma unroll
      for (int k = 0; k < 15; ++k) {
        const float sc = k < 5 ? 1.f : (k < 10 ? s1 : s2);
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            float t = k < 5 ? A[k][c][v] : A[k % 5][c][v] * sc;
            if (a.epi & PTGNN_AMD_EPI_GELU) t = gelu_erf(t);
            y[k][c][v] = t;
            part += colx(c) + v < M ? t : 0.f;
          }
      }
      if (a.epi & PTGNN_AMD_EPI_LAYERNORM) {
        const float width = 15.f * (float)M;
        const float mu = group_sum<LPR>(part) / width;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < 15; ++k)
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              const float dlt = y[k][c][v] - mu;
              q += colx(c) + v < M ? dlt * dlt : 0.f;
            }
        const float rstd = 1.0f / sqrtf(group_sum<LPR>(q) / width + a.ln_eps);
#pragma unroll
        for (int k = 0; k < 15; ++k)
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              const int j = k * M + colx(c) + v;
              if (colx(c) + v < M) y[k][c][v] = (y[k][c][v] - mu) * rstd * a.ln_gamma[j] + a.ln_beta[j];
            }
      }
#pragma unroll
      for (int k = 0; k < 15; ++k) store(orow + k * M, y[k]);
    }
    if constexpr (HAS_ARG) {
      if (a.argmax) store_int(a.argmax + row * (int64_t)M, amx);
      if (a.argmin) store_int(a.argmin + row * (int64_t)M, amn);
    }
  }

  __device__ __forceinline__ void store(float *base, const float (&o)[CH][VEC]) const {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int x = colx(c);
      if (x >= M) continue;
      if constexpr (VEC == 4) *reinterpret_cast<float4 *>(base + x) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
      else base[x] = o[c][0];
    }
  }

  __device__ __forceinline__ void store_int(int32_t *base, const int (&o)[CH][VEC]) const {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int x = colx(c);
      if (x >= M) continue;
      if constexpr (VEC == 4) *reinterpret_cast<int4 *>(base + x) = make_int4(o[c][0], o[c][1], o[c][2], o[c][3]);
      else base[x] = o[c][0];
    }
  }
};

// ------------------------------------------------------------------------------------------------
// forward: one row per lane group (rows up to kPnaLong in-edges)
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPR, int CH, int DST, bool HAS_ARG, bool EPI>
__global__ __launch_bounds__(256) void k_pna_rows(PnaArgs a) {
  constexpr int RPB = 256 / LPR;
  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;
  const int64_t row = tile * RPB + threadIdx.x / LPR;
  if (row >= a.num_nodes) return;   // the whole lane group leaves together (no cross-group shuffles)
  const int beg = a.rowptr[row], end = a.rowptr[row + 1];
  if (end - beg > kPnaLong) return;  // k_pna_long_rows owns it
  PnaRow<VEC, LPR, CH, DST, HAS_ARG, EPI> op(a, threadIdx.x % LPR, blockIdx.y * (LPR * VEC * CH));
  op.pass1(row, beg, end, 1);
  op.set_mean(end - beg);
  op.pass2(row, beg, end, 1);
  op.finish_and_store(row, end - beg);
}

// ------------------------------------------------------------------------------------------------
// forward: one workgroup per long row (more than kPnaLong in-edges)
// ------------------------------------------------------------------------------------------------
// Each workgroup scans 256 consecutive rowptr entries per step and lists the long rows among them in LDS (the list's
// order may vary, every row is still reduced by one workgroup in one fixed order).  Per row: pass 1 over slots
// interleaved across the G lane groups, partials combined by lane group 0 in group order, the mean published through
// LDS, pass 2 likewise, then lane group 0 finishes the row.
template <int VEC, int LPR, int CH, int DST, bool HAS_ARG, bool EPI>
__global__ __launch_bounds__(256) void k_pna_long_rows(PnaArgs a) {
  constexpr int G = 256 / LPR;
  constexpr int W = LPR * VEC * CH;
  __shared__ float p_sum[G * W], p_max[G * W], p_min[G * W];
  __shared__ int p_amax[HAS_ARG ? G * W : 1], p_amin[HAS_ARG ? G * W : 1];
  __shared__ int list[256];
  __shared__ int nlist;
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int cbase = blockIdx.y * W;
  using Op = PnaRow<VEC, LPR, CH, DST, HAS_ARG, EPI>;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.num_nodes; base += (int64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) nlist = 0;
    __syncthreads();
    const int64_t r = base + threadIdx.x;
    if (r < a.num_nodes && a.rowptr[r + 1] - a.rowptr[r] > kPnaLong) list[atomicAdd(&nlist, 1)] = (int)threadIdx.x;
    __syncthreads();
    const int n = nlist;
    for (int k = 0; k < n; ++k) {
      const int64_t row = base + list[k];
      const int beg = a.rowptr[row], end = a.rowptr[row + 1], deg = end - beg;
      Op op(a, g, cbase);
      op.pass1(row, beg + grp, end, G);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int j = grp * W + (g + c * LPR) * VEC + v;
          p_sum[j] = op.sum[c][v]; p_max[j] = op.mx[c][v]; p_min[j] = op.mn[c][v];
          if (HAS_ARG) { p_amax[j] = op.amx[c][v]; p_amin[j] = op.amn[c][v]; }
        }
      __syncthreads();
      if (grp == 0) {
        for (int q = 1; q < G; ++q) {   // fixed combine order => deterministic
          float s[CH][VEC], x[CH][VEC], n2[CH][VEC];
          int ax[CH][VEC], an[CH][VEC];
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              const int j = q * W + (g + c * LPR) * VEC + v;
              s[c][v] = p_sum[j]; x[c][v] = p_max[j]; n2[c][v] = p_min[j];
              ax[c][v] = HAS_ARG ? p_amax[j] : -1; an[c][v] = HAS_ARG ? p_amin[j] : -1;
            }
          op.combine1(s, x, ax, n2, an);
        }
        op.set_mean(deg);
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) p_sum[(g + c * LPR) * VEC + v] = op.mean[c][v];   // publish the mean
      }
      __syncthreads();
      if (grp != 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int v = 0; v < VEC; ++v) op.mean[c][v] = p_sum[(g + c * LPR) * VEC + v];
      }
      op.pass2(row, beg + grp, end, G);
      __syncthreads();   // every group has read the mean
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) p_sum[grp * W + (g + c * LPR) * VEC + v] = op.sq[c][v];
      __syncthreads();
      if (grp == 0) {
        for (int q = 1; q < G; ++q)
#pragma unroll
          for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) op.sq[c][v] += p_sum[q * W + (g + c * LPR) * VEC + v];
        op.finish_and_store(row, deg);
      }
      __syncthreads();   // the partial arrays are free for the next row
    }
    __syncthreads();     // `nlist` has been read by every thread before the next step resets it
  }
}

// ------------------------------------------------------------------------------------------------
// backward (edge form): per row, the gradient of every block folded onto A (g_k = g1 + s*g2 + s'*g3), the relu mask
// recomputed with the forward's fp32 expressions (pos_e = m*m - mean*mean > 0) and its positives P counted per
// column, then per slot, written to message row col[slot]:
//   g_m = gSum + (gMean - gS*2*mean*P) / (d + 1e-5) + [pos]*gS*2*m + gMax*[argmax == slot] + gMin*[argmin == slot]
// with gS = gStd / (2*std).  The std terms are formed in float64 from the fp32 sum (mean = sum / (d + 1e-5), std from
// the same mask): on a degree-1 row [pos]*2*m and 2*mean*P/(d + 1e-5) are ~100x the result they cancel to, and the
// rounding of an fp32 mean / std there moves the gradient by ~1e-5 of its upstream value.  `agg` must hold the
// UNROUNDED A (blocks 0 and 1 are read).  round_mode != 0 (fp16 / bf16 messages): the reference's A is a message-dtype
// tensor, so g_k is rounded to that dtype as autograd accumulates it: h(h(h(g1) + h(s'*g3)) + h(s*g2)).
// ------------------------------------------------------------------------------------------------
template <int VEC, int LPR, int CH>
struct PnaGrad {
  using Row = PnaRow<VEC, LPR, CH, 0, true>;
  Row r;
  float gsum[CH][VEC], gmean[CH][VEC], gstd[CH][VEC], gmax[CH][VEC], gmin[CH][VEC], mm[CH][VEC];
  double meand[CH][VEC], sqd[CH][VEC];
  int P[CH][VEC];

  __device__ __forceinline__ PnaGrad(const PnaArgs &a, int g, int cbase) : r(a, g, cbase) {}

  // the row's per-column terms (sum, mean, arg, block gradients)
  __device__ __forceinline__ void load(int64_t row, int deg) {
    const PnaArgs &a = r.a;
    const int M = r.M;
    const float dd = (float)deg;
    const float s1 = logf(dd + 1.0f) / a.delta;
    const float s2 = 1.0f / (s1 + 1e-3f);
    const double den = (double)(dd + 1e-5f);
    const float *arow = a.agg + row * a.ld_agg;
    const float *grow = a.grad + row * a.ld_grad;
    float gk[5][CH][VEC], t1[CH][VEC], t2[CH][VEC], t3[CH][VEC], sm[CH][VEC];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      r.load_row(grow + k * M, t1);
      r.load_row(grow + (5 + k) * M, t2);
      r.load_row(grow + (10 + k) * M, t3);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (a.round_mode) {   // A was rounded to the message dtype: its gradient is too, accumulated as autograd does
            const int rm = a.round_mode;
            const float h = round_to(round_to(t1[c][v], rm) + round_to(t3[c][v] * s2, rm), rm);
            gk[k][c][v] = round_to(h + round_to(t2[c][v] * s1, rm), rm);
          } else {
            gk[k][c][v] = t1[c][v] + s1 * t2[c][v] + s2 * t3[c][v];
          }
        }
    }
    r.load_row(arow, sm);
    r.load_row(arow + M, r.mean);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int x = r.colx(c);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const bool in = x + v < M;
        r.amx[c][v] = in ? a.amax[row * (int64_t)M + x + v] : -1;
        r.amn[c][v] = in ? a.amin[row * (int64_t)M + x + v] : -1;
        gsum[c][v] = gk[0][c][v];
        gmean[c][v] = gk[1][c][v];
        gmax[c][v] = gk[2][c][v];
        gmin[c][v] = gk[3][c][v];
        gstd[c][v] = gk[4][c][v];
        mm[c][v] = r.mean[c][v] * r.mean[c][v];
        meand[c][v] = (double)sm[c][v] / den;
        sqd[c][v] = 0.0;
        P[c][v] = 0;
      }
    }
  }

  // P and the float64 std sum over the slots beg, beg+stride, ...
  __device__ __forceinline__ void count(int64_t row, int beg, int end, int stride) {
    r.template walk<8>(row, beg, end, stride, [&](const float (&m)[CH][VEC], int, bool valid, int64_t) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float qf = m[c][v] * m[c][v] - mm[c][v];
          const bool pos = valid && qf > 0.f;
          P[c][v] += pos ? 1 : 0;
          // a component the fp32 mask counts never adds less than the forward's fp32 value did
          const double q = (double)m[c][v] * (double)m[c][v] - meand[c][v] * meand[c][v];
          sqd[c][v] += (pos ? (q > 0.0 ? q : (double)qf) : 0.0) + (valid ? 1e-10 : 0.0);
        }
    });
  }

  // -> gsum: gSum + (gMean - gS*2*mean*P) / (d + 1e-5) (float64, rounded once), gstd: gS (float64 kept in sqd)
  __device__ __forceinline__ void finish_terms(int deg) {
    const double den = (double)((float)deg + 1e-5f);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double gs = (double)gstd[c][v] / (2.0 * sqrt(sqd[c][v]));
        sqd[c][v] = gs;
        meand[c][v] = (double)gsum[c][v] + ((double)gmean[c][v] - gs * 2.0 * meand[c][v] * (double)P[c][v]) / den;
      }
  }

  __device__ __forceinline__ void write(int64_t row, int beg, int end, int stride) {
    const PnaArgs &a = r.a;
    r.template walk<8>(row, beg, end, stride, [&](const float (&m)[CH][VEC], int slot, bool valid, int64_t mrow) {
      if (!valid) return;
      float o[CH][VEC];
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const bool pos = m[c][v] * m[c][v] - mm[c][v] > 0.f;
          float t = (float)(pos ? meand[c][v] + sqd[c][v] * 2.0 * (double)m[c][v] : meand[c][v]);
          if (r.amx[c][v] == slot) t = t + gmax[c][v];
          if (r.amn[c][v] == slot) t = t + gmin[c][v];
          o[c][v] = t;
        }
      r.store(a.gmsg + mrow * a.ld_gmsg, o);
    });
  }
};

template <int VEC, int LPR, int CH>
__global__ __launch_bounds__(256) void k_pna_bwd_rows(PnaArgs a) {
  constexpr int RPB = 256 / LPR;
  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;
  const int64_t row = tile * RPB + threadIdx.x / LPR;
  if (row >= a.num_nodes) return;
  const int beg = a.rowptr[row], end = a.rowptr[row + 1];
  if (end == beg || end - beg > kPnaLong) return;   // empty rows have no messages; long rows: k_pna_bwd_long_rows
  PnaGrad<VEC, LPR, CH> op(a, threadIdx.x % LPR, blockIdx.y * (LPR * VEC * CH));
  op.load(row, end - beg);
  op.count(row, beg, end, 1);
  op.finish_terms(end - beg);
  op.write(row, beg, end, 1);
}

// long rows: one workgroup per row; the lane groups count their interleaved slots, the partials (P, the float64 std
// sums) combine in LDS in lane-group order (every group folds the same partials in the same order), then every lane
// group writes its own slots
template <int VEC, int LPR, int CH>
__global__ __launch_bounds__(256) void k_pna_bwd_long_rows(PnaArgs a) {
  constexpr int G = 256 / LPR;
  constexpr int W = LPR * VEC * CH;
  __shared__ int p_cnt[G * W];
  __shared__ double p_sq[G * W];
  __shared__ int list[256];
  __shared__ int nlist;
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int cbase = blockIdx.y * W;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.num_nodes; base += (int64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) nlist = 0;
    __syncthreads();
    const int64_t r = base + threadIdx.x;
    if (r < a.num_nodes && a.rowptr[r + 1] - a.rowptr[r] > kPnaLong) list[atomicAdd(&nlist, 1)] = (int)threadIdx.x;
    __syncthreads();
    const int n = nlist;
    for (int k = 0; k < n; ++k) {
      const int64_t row = base + list[k];
      const int beg = a.rowptr[row], end = a.rowptr[row + 1], deg = end - beg;
      PnaGrad<VEC, LPR, CH> op(a, g, cbase);
      op.load(row, deg);
      op.count(row, beg + grp, end, G);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const int j = grp * W + (g + c * LPR) * VEC + v;
          p_cnt[j] = op.P[c][v];
          p_sq[j] = op.sqd[c][v];
        }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          int cnt = 0;
          double sq = 0.0;
          for (int q = 0; q < G; ++q) {
            const int j = q * W + (g + c * LPR) * VEC + v;
            cnt += p_cnt[j];
            sq += p_sq[j];
          }
          op.P[c][v] = cnt;
          op.sqd[c][v] = sq;
        }
      op.finish_terms(deg);
      op.write(row, beg + grp, end, G);
      __syncthreads();   // the partial arrays are free for the next row
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// launch plumbing
// ------------------------------------------------------------------------------------------------
// lane-group geometry: f(IC<VEC>, IC<LPR>, IC<CH>); one column block is W = LPR*VEC*CH columns (at most 256)
template <typename F>
int pna_geometry(bool vec4, int msg_dim, F f) {
  if (vec4) {
    if (msg_dim <= 64) return f(IC<4>{}, IC<16>{}, IC<1>{});
    if (msg_dim <= 128) return f(IC<4>{}, IC<32>{}, IC<1>{});
    return f(IC<4>{}, IC<64>{}, IC<1>{});
  }
  if (msg_dim <= 64) return f(IC<1>{}, IC<64>{}, IC<1>{});
  return f(IC<1>{}, IC<64>{}, IC<4>{});
}

// one pass over the plan: `rows` (rpb rows per workgroup, rows up to kPnaLong in-edges), then `long_rows` (the rest).
// The kernels arrive as host function pointers: the address of a __global__ function's host stub is its launch handle.
int pna_launch_pair(void (*rows)(PnaArgs), void (*long_rows)(PnaArgs), int rpb, const PnaArgs &a0, int col_blocks,
                    hipStream_t stream) {
  PnaArgs a = a0;
  a.num_tiles = (a.num_nodes + rpb - 1) / rpb;
  dim3 grid((unsigned)xcd_padded_blocks(a.num_tiles), (unsigned)col_blocks);
  rows<<<grid, 256, 0, stream>>>(a);
  PTGNN_LAUNCH_CHECK();
  const int64_t lb = (a.num_nodes + 255) / 256;
  dim3 lgrid((unsigned)(lb < 1024 ? lb : 1024), (unsigned)col_blocks);
  long_rows<<<lgrid, 256, 0, stream>>>(a);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

template <int VEC, int LPR, int CH, int DST, bool HAS_ARG, bool EPI = false>
int pna_launch(const PnaArgs &a, int col_blocks, hipStream_t stream) {
  return pna_launch_pair(k_pna_rows<VEC, LPR, CH, DST, HAS_ARG, EPI>, k_pna_long_rows<VEC, LPR, CH, DST, HAS_ARG, EPI>,
                         256 / LPR, a, col_blocks, stream);
}

template <int VEC, int LPR, int CH>
int pna_backward_launch(const PnaArgs &a, int col_blocks, hipStream_t stream) {
  return pna_launch_pair(k_pna_bwd_rows<VEC, LPR, CH>, k_pna_bwd_long_rows<VEC, LPR, CH>, 256 / LPR, a, col_blocks,
                         stream);
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_pna_aggregate_f32(const float *ysrc, int64_t ld_y, const float *ydst, int64_t ld_yd,
                                           const int32_t *rowptr, const int32_t *col, int32_t type_bits,
                                           int64_t num_nodes, int32_t msg_dim, float delta, int epilogue,
                                           const float *ln_gamma, const float *ln_beta, float ln_eps,
                                           int32_t round_mode, float *out, int64_t ld_out, int32_t *argmax,
                                           int32_t *argmin, float *agg_out, int64_t num_edges, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && num_edges >= 0 && msg_dim > 0 && msg_dim < (1 << 20), PTGNN_AMD_EINVAL,
                "pna_aggregate: bad sizes");
  PTGNN_REQUIRE(num_nodes < ((int64_t)1 << 31) && num_edges < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "pna_aggregate: more than 2^31 rows or edges");
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "pna_aggregate: bad type_bits");
  PTGNN_REQUIRE(epilogue >= 0 && epilogue <= PTGNN_AMD_EPI_GELU_LAYERNORM, PTGNN_AMD_EINVAL,
                "pna_aggregate: unknown epilogue %d", epilogue);
  PTGNN_REQUIRE(round_mode >= 0 && round_mode <= 2, PTGNN_AMD_EINVAL, "pna_aggregate: unknown round_mode %d",
                round_mode);
  PTGNN_REQUIRE(delta != 0.f, PTGNN_AMD_EINVAL, "pna_aggregate: delta must be non-zero");
  PTGNN_REQUIRE((argmax == nullptr) == (argmin == nullptr), PTGNN_AMD_EINVAL,
                "pna_aggregate: argmax and argmin are asked for together");
  PTGNN_REQUIRE(agg_out == nullptr || epilogue == 0, PTGNN_AMD_EUNSUPPORTED,
                "pna_aggregate: agg_out with an epilogue");
  PTGNN_REQUIRE(argmax == nullptr || (ydst == nullptr && epilogue == 0), PTGNN_AMD_EUNSUPPORTED,
                "pna_aggregate: argmax / argmin with a destination term or an epilogue");
  if (num_nodes == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && out && (ysrc || num_edges == 0), PTGNN_AMD_EINVAL, "pna_aggregate: null pointer");
  PTGNN_REQUIRE(ld_out >= 15 * (int64_t)msg_dim && ld_y >= msg_dim && (!ydst || ld_yd >= msg_dim), PTGNN_AMD_EINVAL,
                "pna_aggregate: bad leading dimension");
  PTGNN_REQUIRE(!(epilogue & PTGNN_AMD_EPI_LAYERNORM) || (ln_gamma && ln_beta), PTGNN_AMD_EINVAL,
                "pna_aggregate: LayerNorm epilogue without its parameters");
  const bool vec4 = msg_dim % 4 == 0 && ld_y % 4 == 0 && ld_out % 4 == 0 && (!ysrc || aligned16(ysrc)) &&
                    aligned16(out) && (!ydst || (ld_yd % 4 == 0 && aligned16(ydst))) &&
                    (!argmax || (aligned16(argmax) && aligned16(argmin))) && (!agg_out || aligned16(agg_out));
  const int col_blocks = (msg_dim + 255) / 256;
  PTGNN_REQUIRE(epilogue == 0 || col_blocks == 1, PTGNN_AMD_EUNSUPPORTED,
                "pna_aggregate: the GELU / LayerNorm epilogue supports msg_dim <= 256 (got %d)", msg_dim);
  PnaArgs a{};
  a.ysrc = ysrc ? ysrc : reinterpret_cast<const float *>(rowptr);   // never read without edges
  a.ydst = ydst; a.ld_y = ld_y; a.ld_yd = ld_yd;
  a.rowptr = rowptr; a.col = col; a.type_bits = type_bits; a.num_nodes = num_nodes; a.msg_dim = msg_dim;
  a.delta = delta; a.epi = epilogue; a.ln_gamma = ln_gamma; a.ln_beta = ln_beta; a.ln_eps = ln_eps;
  a.round_mode = round_mode; a.out = out; a.ld_out = ld_out; a.argmax = argmax; a.argmin = argmin; a.agg_out = agg_out;
  hipStream_t stream = (hipStream_t)stream_;
  const int dst = ydst == nullptr ? 0 : (type_bits == 0 ? 2 : 1);
  const int rc = pna_geometry(vec4, msg_dim, [&](auto V, auto L, auto C) {
    constexpr int VV = decltype(V)::value, LL = decltype(L)::value, CC = decltype(C)::value;
    if (argmax) return pna_launch<VV, LL, CC, 0, true>(a, col_blocks, stream);
    if (epilogue) {
      if (dst == 1) return pna_launch<VV, LL, CC, 1, false, true>(a, col_blocks, stream);
      if (dst == 2) return pna_launch<VV, LL, CC, 2, false, true>(a, col_blocks, stream);
      return pna_launch<VV, LL, CC, 0, false, true>(a, col_blocks, stream);
    }
    if (dst == 1) return pna_launch<VV, LL, CC, 1, false>(a, col_blocks, stream);
    if (dst == 2) return pna_launch<VV, LL, CC, 2, false>(a, col_blocks, stream);
    return pna_launch<VV, LL, CC, 0, false>(a, col_blocks, stream);
  });
  if (rc == PTGNN_AMD_OK) count_launch(PTGNN_AMD_KERNEL_PNA_AGGREGATE);
  return rc;
}

extern "C" int ptgnn_amd_pna_aggregate_backward_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr,
                                                    const int32_t *col, int64_t num_nodes, int32_t msg_dim,
                                                    float delta, const float *agg, int64_t ld_agg,
                                                    const int32_t *argmax, const int32_t *argmin, const float *grad,
                                                    int64_t ld_grad, float *grad_msg, int64_t ld_grad_msg,
                                                    int32_t round_mode, int64_t num_edges, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && num_edges >= 0 && msg_dim > 0 && msg_dim < (1 << 20), PTGNN_AMD_EINVAL,
                "pna_aggregate_backward: bad sizes");
  PTGNN_REQUIRE(num_nodes < ((int64_t)1 << 31) && num_edges < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "pna_aggregate_backward: more than 2^31 rows or edges");
  PTGNN_REQUIRE(delta != 0.f, PTGNN_AMD_EINVAL, "pna_aggregate_backward: delta must be non-zero");
  PTGNN_REQUIRE(round_mode >= 0 && round_mode <= 2, PTGNN_AMD_EINVAL,
                "pna_aggregate_backward: unknown round_mode %d", round_mode);
  if (num_nodes == 0 || num_edges == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(msg && rowptr && col && agg && argmax && argmin && grad && grad_msg, PTGNN_AMD_EINVAL,
                "pna_aggregate_backward: null pointer");
  PTGNN_REQUIRE(ld_msg >= msg_dim && ld_agg >= 5 * (int64_t)msg_dim && ld_grad >= 15 * (int64_t)msg_dim &&
                    ld_grad_msg >= msg_dim,
                PTGNN_AMD_EINVAL, "pna_aggregate_backward: bad leading dimension");
  const bool vec4 = msg_dim % 4 == 0 && ld_msg % 4 == 0 && ld_agg % 4 == 0 && ld_grad % 4 == 0 &&
                    ld_grad_msg % 4 == 0 && aligned16(msg) && aligned16(agg) && aligned16(grad) &&
                    aligned16(grad_msg);
  PnaArgs a{};
  a.ysrc = msg; a.ydst = nullptr; a.ld_y = ld_msg; a.ld_yd = ld_msg;
  a.rowptr = rowptr; a.col = col; a.type_bits = 0; a.num_nodes = num_nodes; a.msg_dim = msg_dim; a.delta = delta;
  a.agg = agg; a.ld_agg = ld_agg; a.amax = argmax; a.amin = argmin; a.grad = grad; a.ld_grad = ld_grad;
  a.gmsg = grad_msg; a.ld_gmsg = ld_grad_msg; a.round_mode = round_mode;
  hipStream_t stream = (hipStream_t)stream_;
  const int col_blocks = (msg_dim + 255) / 256;
  const int rc = pna_geometry(vec4, msg_dim, [&](auto V, auto L, auto C) {
    return pna_backward_launch<decltype(V)::value, decltype(L)::value, decltype(C)::value>(a, col_blocks, stream);
  });
  if (rc == PTGNN_AMD_OK) count_launch(PTGNN_AMD_KERNEL_PNA_AGGREGATE_BACKWARD);
  return rc;
}
