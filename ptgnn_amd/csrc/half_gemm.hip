// Opt-in reduced-precision dense blocks of the GGNN layer: 16-bit (bf16 / fp16) operands on the matrix cores
// (v_mfma_f32_32x32x16_{bf16,f16}), fp32 everywhere else.  The C-ABI entry points
//   ptgnn_amd_half_linear   : y = act(rnd(x) rnd(W)^T + b)
//   ptgnn_amd_half_gru_cell : h' = GRUCell(a, h) with rnd(a), rnd(h), rnd(W_ih), rnd(W_hh) in the gate GEMMs
//   ptgnn_amd_half_supported: the shape check of the two, no device needed
// Contracts + reference lines: include/ptgnn_amd.h.
//
// States stay fp32 in HBM.  A lane loads the 8 consecutive floats of its MFMA A fragment (lane l = row l & 31,
// k = 8 (l >> 5) + j: cdna_hip_programming.md section 3) as two dwordx4 and rounds them to the 16-bit type in registers
// (fptrunc: round to nearest even, what tensor.to(dtype) does; never a truncating pack); the weights arrive already
// rounded by the host as 16-bit arrays, so a lane's B fragment (column l & 31 of W^T = row l & 31 of W, the same 8 k) is
// one dwordx4.  In k_half_linear and k_half_gru neither operand goes through LDS: the fragment IS the memory order.
// Products of two 16-bit values are exact in fp32; accumulation, bias, activation, gate math and the stores are fp32.
//
// One wave owns 32 rows: 32 x 128 output columns of the Linear (4 accumulators), 32 x 32 or 32 x 64 state features of the
// GRU (4 accumulators -- r, z, i_n, h_n -- per 32 features; r and z are ONE chain over K = M + H).  A workgroup is four
// such waves over consecutive 32-row units and the same columns, so their weight reads hit the same cache lines.
// The GGNN widths of the GRU (M, H in {64, 128}) take k_half_gru_ws further down: weights stationary in registers, row
// panels rounded once into LDS.  Measured: profiles/half_inputs_notes.md.
//
// Row independence: the K order of a row's chains is fixed (k ascending in steps of 16, the a phase before the h
// phase), every lane of a row runs the same instruction stream, and the gate math is individually rounded per element
// (no contraction), so the bits of output row r depend on row r and the weights only -- not on the number of rows, the
// row's position in its tile or the launch geometry.  ops.aggregate_gru relies on it.
//
// No atomics, no inline assembly; every store is a plain C++ assignment.
#include "half16.h"
#include "stream_gemm.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

constexpr int kLinTiles = 4;   // 32-column tiles per wave of the Linear

template <int DT>
__global__ __launch_bounds__(256) void k_half_linear(const float *__restrict__ x, int64_t rows, int K, int64_t ld_x,
                                                     const uint16_t *__restrict__ w, int n_out,
                                                     const float *__restrict__ bias, int act, float *__restrict__ y,
                                                     int64_t ld_y, int col_groups) {
  using H = Half16<DT>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, hi = lane >> 5;
  const int64_t row0 = ((int64_t)(blockIdx.x / col_groups) * 4 + wave) * 32;
  if (row0 >= rows) return;                       // no barrier in this kernel
  const int col0 = (int)(blockIdx.x % col_groups) * (32 * kLinTiles);
  const int tiles = (n_out - col0) / 32 < kLinTiles ? (n_out - col0) / 32 : kLinTiles;   // >= 1

  f32x16 acc[kLinTiles];
#pragma unroll
  for (int t = 0; t < kLinTiles; ++t) zero(acc[t]);

  // rows past the end read the last valid row (never stored); column tiles past the end recompute the last valid one
  int64_t arow = row0 + li;
  arow = arow < rows ? arow : rows - 1;
  const float *ap = x + arow * ld_x + 8 * hi;
  const uint16_t *bp[kLinTiles];
#pragma unroll
  for (int t = 0; t < kLinTiles; ++t) {
    const int tc = t < tiles ? t : tiles - 1;
    bp[t] = w + (int64_t)(col0 + tc * 32 + li) * K + 8 * hi;
  }
  for (int kk = 0; kk < K; kk += 32) {           // K % 32 == 0: two MFMA k-steps per trip
#pragma unroll
    for (int k0 = kk; k0 < kk + 32; k0 += 16) {
      const typename H::vec a = round8<DT>(ap + k0);
#pragma unroll
      for (int t = 0; t < kLinTiles; ++t) acc[t] = H::mfma(a, load8<DT>(bp[t] + k0), acc[t]);
    }
  }

#pragma unroll
  for (int t = 0; t < kLinTiles; ++t) {
    if (t < tiles) {
      const int col = col0 + t * 32 + li;
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = row0 + frag_row(r, hi);
        if (row < rows) y[row * ld_y + col] = act_runtime(acc[t][r] + bv, act);
      }
    }
  }
}

// Gate math of one element: the streaming fp32 cell's expressions (stream_gemm.hip gru_epilogue: hardware exp2 / rcp
// sigmoid and tanh), individually rounded -- both cells share one bar against a float64 reference.
__device__ __forceinline__ float gru_gate(float ar, float az, float an, float ah, float hprev, float bir, float biz,
                                          float bin, float bhr, float bhz, float bhn) {
#pragma clang fp contract(off)
  const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(((ar + bir) + bhr) * -1.4426950408889634f));
  const float z = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(((az + biz) + bhz) * -1.4426950408889634f));
  const float hn = ah + bhn;
  const float pre = (an + bin) + r * hn;
  const float n = 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pre * -2.8853900817779268f)) - 1.0f;
  return (1.0f - z) * n + z * hprev;
}

template <int DT, int NF>
__global__ __launch_bounds__(256) void k_half_gru(const float *__restrict__ a, int64_t ld_a,
                                                  const float *__restrict__ h, int64_t ld_h,
                                                  const uint16_t *__restrict__ w_ih, const uint16_t *__restrict__ w_hh,
                                                  const float *__restrict__ b_ih, const float *__restrict__ b_hh,
                                                  int64_t n, int M, int Hd, float *__restrict__ out, int64_t ld_out,
                                                  int col_groups) {
  using H = Half16<DT>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, hi = lane >> 5;
  const int64_t row0 = ((int64_t)(blockIdx.x / col_groups) * 4 + wave) * 32;
  if (row0 >= n) return;                          // no barrier in this kernel
  const int j0 = (int)(blockIdx.x % col_groups) * (32 * NF);   // Hd % (32 NF) == 0: every tile is whole

  f32x16 acc[NF][4];   // r, z, i_n, h_n
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int g = 0; g < 4; ++g) zero(acc[f][g]);

  int64_t arow = row0 + li;
  arow = arow < n ? arow : n - 1;                 // rows past the end read the last valid row, never stored
  {  // phase 0: K over the aggregated messages (a, W_ih) -> r, z, i_n
    const float *ap = a + arow * ld_a + 8 * hi;
    const uint16_t *bp = w_ih + (int64_t)(j0 + li) * M + 8 * hi;
    for (int kk = 0; kk < M; kk += 32) {         // M % 32 == 0: two MFMA k-steps per trip
#pragma unroll
      for (int k0 = kk; k0 < kk + 32; k0 += 16) {
        const typename H::vec av = round8<DT>(ap + k0);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int g = 0; g < 3; ++g)
            acc[f][g] = H::mfma(av, load8<DT>(bp + ((int64_t)g * Hd + f * 32) * M + k0), acc[f][g]);
      }
    }
  }
  {  // phase 1: K over the previous state (h, W_hh) -> r, z, h_n
    const float *ap = h + arow * ld_h + 8 * hi;
    const uint16_t *bp = w_hh + (int64_t)(j0 + li) * Hd + 8 * hi;
    for (int kk = 0; kk < Hd; kk += 32) {
#pragma unroll
      for (int k0 = kk; k0 < kk + 32; k0 += 16) {
        const typename H::vec av = round8<DT>(ap + k0);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            const int slot = g == 2 ? 3 : g;
            acc[f][slot] = H::mfma(av, load8<DT>(bp + ((int64_t)g * Hd + f * 32) * Hd + k0), acc[f][slot]);
          }
      }
    }
  }

#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int j = j0 + f * 32 + li;
    const float bir = b_ih[j], biz = b_ih[Hd + j], bin = b_ih[2 * Hd + j];
    const float bhr = b_hh[j], bhz = b_hh[Hd + j], bhn = b_hh[2 * Hd + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + frag_row(r, hi);
      if (row < n) {
        const float hprev = h[row * ld_h + j];    // the UNROUNDED state (L2-hot: phase 1 just streamed the row)
        out[row * ld_out + j] = gru_gate(acc[f][0][r], acc[f][1][r], acc[f][2][r], acc[f][3][r], hprev, bir, biz, bin,
                                         bhr, bhz, bhn);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The GRU cell, weight-stationary, for the GGNN widths (M, H in {64, 128}; KA = M / 16, KH = H / 16 MFMA k-steps).
// k_half_gru above pays one cache-line look-up per lane and load (a lane is a ROW of the operand); here
//   * a wave keeps the weights of its 32 state features in registers for the whole launch: 3 gates x (KA + KH) fragments
//     (192 VGPRs at M = H = 128; one wave per SIMD), loaded once;
//   * a workgroup's four waves are the H / 32 feature slices of 32 (H = 128) or 64 (H = 64) rows, and walk the row panels
//     of the launch workgroup-strided; a panel's [a | h] rows are loaded ONCE, coalesced (a thread's float4s are
//     consecutive in a row), rounded to the 16-bit type and parked in LDS (row stride (M + H + 8) x 2 bytes: an odd
//     number of 16-byte units, so the ds_read_b128 fragment reads of 16 consecutive rows hit 64 distinct banks);
//   * the next panel's loads are issued before the current panel's MFMAs and land in the other LDS buffer after them:
//     one barrier per panel.
// Same chains as k_half_gru (k ascending, the a phase before the h phase, one accumulator per gate) and the same gate
// math: the two kernels give the same bits, so which one runs (a function of M and H alone) is not observable.
// ---------------------------------------------------------------------------------------------
template <int DT, int KA, int KH>
__global__ __launch_bounds__(256) void k_half_gru_ws(const float *__restrict__ a, int64_t ld_a,
                                                     const float *__restrict__ h, int64_t ld_h,
                                                     const uint16_t *__restrict__ w_ih,
                                                     const uint16_t *__restrict__ w_hh,
                                                     const float *__restrict__ b_ih, const float *__restrict__ b_hh,
                                                     int64_t n, float *__restrict__ out, int64_t ld_out,
                                                     int64_t num_panels) {
  using H = Half16<DT>;
  using vec = typename H::vec;
  using half4 = __attribute__((ext_vector_type(4))) typename H::elem;
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  constexpr int M = 16 * KA, Hd = 16 * KH, KS = KA + KH, KT = M + Hd;
  constexpr int S = Hd / 32;             // feature slices = waves per row unit (2 or 4)
  constexpr int PR = 32 * (4 / S);       // rows per panel (64 or 32)
  constexpr int LD = KT + 8;             // LDS row stride in 16-bit elements
  constexpr int RV = KT / 4;             // float4 per panel row
  constexpr int NV = PR * RV / 256;      // float4 per thread and panel
  static_assert(PR * RV % 256 == 0 && (LD / 8) % 2 == 1, "panel shape");
  __shared__ __attribute__((aligned(16))) uint16_t panel[2][PR * LD];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, hi = lane >> 5;
  const int slice = wave % S, ru = wave / S;
  const int j = slice * 32 + li;

  // this wave's weights, once: bw[g][ks] = rows g Hd + j of [W_ih | W_hh], k-step ks
  vec bw[3][KS];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int ks = 0; ks < KA; ++ks) bw[g][ks] = load8<DT>(w_ih + (int64_t)(g * Hd + j) * M + ks * 16 + 8 * hi);
#pragma unroll
    for (int ks = 0; ks < KH; ++ks) bw[g][KA + ks] = load8<DT>(w_hh + (int64_t)(g * Hd + j) * Hd + ks * 16 + 8 * hi);
  }
  const float bir = b_ih[j], biz = b_ih[Hd + j], bin = b_ih[2 * Hd + j];
  const float bhr = b_hh[j], bhz = b_hh[Hd + j], bhn = b_hh[2 * Hd + j];

  float4 stage[NV];
  auto fetch = [&](int64_t p) {          // panel p's [a | h] rows -> registers (rows past n: the last valid row)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      const int r = v / RV, c = (v % RV) * 4;
      int64_t row = p * PR + r;
      row = row < n ? row : n - 1;
      const float *src = c < M ? a + row * ld_a + c : h + row * ld_h + (c - M);
      stage[i] = *reinterpret_cast<const float4 *>(src);
    }
  };
  auto park = [&](int buf) {             // registers -> rounded 16-bit panel in LDS
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      const int r = v / RV, c = (v % RV) * 4;
      const f32x4 f = {stage[i].x, stage[i].y, stage[i].z, stage[i].w};
      *reinterpret_cast<half4 *>(&panel[buf][r * LD + c]) = __builtin_convertvector(f, half4);
    }
  };

  int64_t p = blockIdx.x;
  if (p >= num_panels) return;           // whole workgroup: before any barrier
  fetch(p);
  park(0);
  __syncthreads();
  int cur = 0;
  for (; p < num_panels; p += gridDim.x) {
    const int64_t next = p + gridDim.x;
    fetch(next < num_panels ? next : p);   // no branch around the loads; the last trip re-reads its own panel

    f32x16 acc[4];   // r, z, i_n, h_n
#pragma unroll
    for (int g = 0; g < 4; ++g) zero(acc[g]);
    const uint16_t *ap = &panel[cur][(ru * 32 + li) * LD + 8 * hi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const vec av = *reinterpret_cast<const vec *>(ap + ks * 16);
      acc[0] = H::mfma(av, bw[0][ks], acc[0]);
      acc[1] = H::mfma(av, bw[1][ks], acc[1]);
      if (ks < KA) acc[2] = H::mfma(av, bw[2][ks], acc[2]);
      else         acc[3] = H::mfma(av, bw[2][ks], acc[3]);
    }
    const int64_t row0 = p * PR + ru * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + frag_row(r, hi);
      if (row < n) {
        const float hprev = h[row * ld_h + j];    // the UNROUNDED state
        out[row * ld_out + j] = gru_gate(acc[0][r], acc[1][r], acc[2][r], acc[3][r], hprev, bir, biz, bin, bhr, bhz, bhn);
      }
    }
    park(cur ^ 1);
    __syncthreads();                     // the other buffer is complete; everyone is done reading this one
    cur ^= 1;
  }
}

bool shape_ok(int kind, int32_t k_or_m, int32_t n_out_or_hd) {
  if (kind == PTGNN_AMD_HALF_KIND_LINEAR)
    return k_or_m > 0 && k_or_m % 32 == 0 && k_or_m <= 1024 && n_out_or_hd > 0 && n_out_or_hd % 32 == 0;
  if (kind == PTGNN_AMD_HALF_KIND_GRU)
    return k_or_m > 0 && k_or_m % 32 == 0 && k_or_m <= 1024 && n_out_or_hd > 0 && n_out_or_hd % 32 == 0 &&
           n_out_or_hd <= 1024;
  return false;
}

// a float matrix the fragment loads can read: 16-byte aligned base, rows a multiple of 16 bytes apart
bool rows16(const void *p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }
bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_half_supported(int kind, int32_t k_or_m, int32_t n_out_or_hd, int dtype) {
  return dtype_ok(dtype) && shape_ok(kind, k_or_m, n_out_or_hd) ? 1 : 0;
}

extern "C" int ptgnn_amd_half_linear(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w,
                                     int32_t n_out, const float *bias, int act, int dtype, float *y, int64_t ld_y,
                                     void *stream_) {
  PTGNN_REQUIRE(rows >= 0 && k > 0 && n_out > 0, PTGNN_AMD_EINVAL, "half_linear: bad sizes");
  PTGNN_REQUIRE(act >= 0 && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "half_linear: bad act");
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "half_linear: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", dtype);
  PTGNN_REQUIRE(shape_ok(PTGNN_AMD_HALF_KIND_LINEAR, k, n_out), PTGNN_AMD_EUNSUPPORTED,
                "half_linear: k=%d n_out=%d: needs k %% 32 == 0, k <= 1024, n_out %% 32 == 0", k, n_out);
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && w && y && ld_x >= k && ld_y >= n_out, PTGNN_AMD_EINVAL, "half_linear: null/ld");
  PTGNN_REQUIRE(rows16(x, ld_x) && aligned16(w) && aligned4(y) && (!bias || aligned4(bias)), PTGNN_AMD_EUNSUPPORTED,
                "half_linear: x and w must be 16-byte aligned with ld_x %% 4 == 0 (ld_x=%lld), y and bias float-aligned",
                (long long)ld_x);
  const int col_groups = (n_out + 32 * kLinTiles - 1) / (32 * kLinTiles);
  const int64_t blocks = (rows + 127) / 128 * col_groups;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "half_linear: too many tiles");
  hipStream_t st = (hipStream_t)stream_;
  const uint16_t *w16 = static_cast<const uint16_t *>(w);
  if (dtype == PTGNN_AMD_HALF_BF16)
    k_half_linear<PTGNN_AMD_HALF_BF16><<<(unsigned)blocks, 256, 0, st>>>(x, rows, k, ld_x, w16, n_out, bias, act, y,
                                                                         ld_y, col_groups);
  else
    k_half_linear<PTGNN_AMD_HALF_F16><<<(unsigned)blocks, 256, 0, st>>>(x, rows, k, ld_x, w16, n_out, bias, act, y,
                                                                        ld_y, col_groups);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_HALF_LINEAR);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_half_gru_cell(const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                                       const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m,
                                       int32_t hd, int dtype, float *out, int64_t ld_out, void *stream_) {
  PTGNN_REQUIRE(n >= 0 && m > 0 && hd > 0, PTGNN_AMD_EINVAL, "half_gru_cell: bad sizes");
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "half_gru_cell: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16",
                dtype);
  PTGNN_REQUIRE(shape_ok(PTGNN_AMD_HALF_KIND_GRU, m, hd), PTGNN_AMD_EUNSUPPORTED,
                "half_gru_cell: m=%d hd=%d: needs m %% 32 == 0, hd %% 32 == 0, both <= 1024", m, hd);
  if (n == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(a && h && w_ih && w_hh && b_ih && b_hh && out, PTGNN_AMD_EINVAL, "half_gru_cell: null");
  PTGNN_REQUIRE(ld_a >= m && ld_h >= hd && ld_out >= hd, PTGNN_AMD_EINVAL, "half_gru_cell: bad ld");
  PTGNN_REQUIRE(out != h, PTGNN_AMD_EINVAL, "half_gru_cell: in-place update is not supported");
  PTGNN_REQUIRE(rows16(a, ld_a) && rows16(h, ld_h) && aligned16(w_ih) && aligned16(w_hh) && aligned4(out) &&
                    aligned4(b_ih) && aligned4(b_hh),
                PTGNN_AMD_EUNSUPPORTED,
                "half_gru_cell: a, h and the weights must be 16-byte aligned with ld %% 4 == 0 (ld_a=%lld, ld_h=%lld), "
                "out and the biases float-aligned", (long long)ld_a, (long long)ld_h);
  const int nf = hd % 64 == 0 ? 2 : 1;
  const int col_groups = hd / (32 * nf);
  const int64_t blocks = (n + 127) / 128 * col_groups;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "half_gru_cell: too many tiles");
  hipStream_t st = (hipStream_t)stream_;
  const uint16_t *wi = static_cast<const uint16_t *>(w_ih), *wh = static_cast<const uint16_t *>(w_hh);
  if ((m == 64 || m == 128) && (hd == 64 || hd == 128)) {   // the GGNN widths: weight-stationary (same bits)
    const int64_t num_panels = (n + (hd == 128 ? 31 : 63)) / (hd == 128 ? 32 : 64);
    const int64_t cus = num_compute_units();
    const unsigned grid = (unsigned)(num_panels < cus ? num_panels : cus);
#define PTGNN_HALF_GRU_WS(DT, KA, KH) \
  k_half_gru_ws<DT, KA, KH><<<grid, 256, 0, st>>>(a, ld_a, h, ld_h, wi, wh, b_ih, b_hh, n, out, ld_out, num_panels)
#define PTGNN_HALF_GRU_WS_DT(DT)                                        \
  do {                                                                  \
    if (m == 64 && hd == 64) PTGNN_HALF_GRU_WS(DT, 4, 4);               \
    else if (m == 128 && hd == 64) PTGNN_HALF_GRU_WS(DT, 8, 4);         \
    else if (m == 64 && hd == 128) PTGNN_HALF_GRU_WS(DT, 4, 8);         \
    else PTGNN_HALF_GRU_WS(DT, 8, 8);                                   \
  } while (0)
    if (dtype == PTGNN_AMD_HALF_BF16) PTGNN_HALF_GRU_WS_DT(PTGNN_AMD_HALF_BF16);
    else PTGNN_HALF_GRU_WS_DT(PTGNN_AMD_HALF_F16);
#undef PTGNN_HALF_GRU_WS_DT
#undef PTGNN_HALF_GRU_WS
    PTGNN_LAUNCH_CHECK();
    count_launch(PTGNN_AMD_KERNEL_HALF_GRU);
    return PTGNN_AMD_OK;
  }
#define PTGNN_HALF_GRU(DT, NF)                                                                                     \
  k_half_gru<DT, NF><<<(unsigned)blocks, 256, 0, st>>>(a, ld_a, h, ld_h, wi, wh, b_ih, b_hh, n, m, hd, out, ld_out, \
                                                       col_groups)
  if (dtype == PTGNN_AMD_HALF_BF16) { if (nf == 2) PTGNN_HALF_GRU(PTGNN_AMD_HALF_BF16, 2); else PTGNN_HALF_GRU(PTGNN_AMD_HALF_BF16, 1); }
  else                              { if (nf == 2) PTGNN_HALF_GRU(PTGNN_AMD_HALF_F16, 2); else PTGNN_HALF_GRU(PTGNN_AMD_HALF_F16, 1); }
#undef PTGNN_HALF_GRU
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_HALF_GRU);
  return PTGNN_AMD_OK;
}
