// Opt-in reduced-precision dense blocks of the GGNN layer: 16-bit (bf16 / fp16) operands on the matrix cores
// (v_mfma_f32_32x32x16_{bf16,f16}), fp32 everywhere else.  The C-ABI entry points
//   ptgnn_amd_half_linear   : y = act(rnd(x) rnd(W)^T + b)
//   ptgnn_amd_half_gru_cell : h' = GRUCell(a, h) with rnd(a), rnd(h), rnd(W_ih), rnd(W_hh) in the gate GEMMs
//   ptgnn_amd_half_supported: the shape check of the two (and of csrc/wgrad16.hip's kind), no device needed
// and the training forms, one template flag each on the same kernels (same chains, same bits):
//   ptgnn_amd_gru_cell_train16: ptgnn_amd_half_gru_cell that also writes gates [n, 4 hd] = r | z | n | gh_n
//   ptgnn_amd_linear_add16    : ptgnn_amd_half_linear plus an fp32 addend in the store epilogue
// Contracts + reference lines: include/ptgnn_amd.h.  Operands, the chain, the per-wave tile and the rounded LDS panel:
// half16.h.  Bias, activation, gate math and the stores are fp32.
//
// One wave owns 32 rows: 32 x 128 output columns of the Linear (one wave_tile of 4 accumulators), 32 x 32 or 32 x 64
// state features of the GRU (4 accumulators -- r, z, i_n, h_n -- per 32 features; r and z are ONE chain over K = M + H).
// A workgroup is four such waves over consecutive 32-row units and the same columns, so their weight reads hit the same
// cache lines.  The GGNN widths of the GRU (M, H in {64, 128}) take k_half_gru_ws further down: weights stationary in
// registers, row panels rounded once into LDS.  Measured: profiles/half_inputs_notes.md.
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

// ADD: y = act(..) + addend (fp32 [rows, n_out], ld_add) in the store epilogue: ptgnn_amd_linear_add16
template <int DT, bool ADD>
__global__ __launch_bounds__(256) void k_half_linear(const float *__restrict__ x, int64_t rows, int K, int64_t ld_x,
                                                     const uint16_t *__restrict__ w, int n_out,
                                                     const float *__restrict__ bias, int act, float *__restrict__ y,
                                                     int64_t ld_y, int col_groups, const float *__restrict__ addend,
                                                     int64_t ld_add) {
  const int wave = threadIdx.x >> 6, li = frag_li(), hi = frag_hi();
  const int64_t row0 = ((int64_t)(blockIdx.x / col_groups) * 4 + wave) * 32;
  if (row0 >= rows) return;                       // no barrier in this kernel
  const int col0 = (int)(blockIdx.x % col_groups) * (32 * kLinTiles);
  const int tiles = (n_out - col0) / 32 < kLinTiles ? (n_out - col0) / 32 : kLinTiles;   // >= 1

  int64_t arow = row0 + li;
  arow = arow < rows ? arow : rows - 1;           // rows past the end read the last valid row, never stored
  f32x16 acc[kLinTiles];
  wave_tile<DT>(x + arow * ld_x, w, K, col0, tiles, acc);

#pragma unroll
  for (int t = 0; t < kLinTiles; ++t) {
    if (t < tiles) {
      const int col = col0 + t * 32 + li;
      const float bv = bias ? bias[col] : 0.f;
      // not for_frag_rows: under it the 16 row addresses are hoisted out of the tile loop (76 -> 102 VGPRs), measured
      // 0.7 % slower at the cfg3 shape (profiles/half16_refactor_notes.md)
      float av[16];
      // ADD: the tile's 16 addends in flight together (rows past the end: the last row, never stored).  Loaded inside
      // the store loop they were 16 dependent round trips per tile: 202 -> 117 us at 119 k rows, K = 384 -> 128
      // (profiles/half_training_notes.md).
      if constexpr (ADD) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = row0 + frag_row(r, hi);
          av[r] = addend[(row < rows ? row : rows - 1) * ld_add + col];
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = row0 + frag_row(r, hi);
        if (row < rows) {
          const float v = act_runtime(acc[t][r] + bv, act);
          if constexpr (ADD) y[row * ld_y + col] = v + av[r];
          else y[row * ld_y + col] = v;
        }
      }
    }
  }
}

// Gate math of one element: the streaming fp32 cell's expressions (stream_gemm.hip gru_epilogue: hardware exp2 / rcp
// sigmoid and tanh), individually rounded -- both cells share one bar against a float64 reference.
// TRAIN: the values the gate math used go to gp[0], gp[hd], gp[2 hd], gp[3 hd] = r, z, n, gh_n (the gates row of the fp32
// training cell: ptgnn_amd_gru_cell_backward_gates_f32 reads them); the returned bits are those of the inference form.
template <bool TRAIN>
__device__ __forceinline__ float gru_gate(float ar, float az, float an, float ah, float hprev, float bir, float biz,
                                          float bin, float bhr, float bhz, float bhn, float *__restrict__ gp, int hd) {
#pragma clang fp contract(off)
  const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(((ar + bir) + bhr) * -1.4426950408889634f));
  const float z = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(((az + biz) + bhz) * -1.4426950408889634f));
  const float hn = ah + bhn;
  const float pre = (an + bin) + r * hn;
  const float n = 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pre * -2.8853900817779268f)) - 1.0f;
  if constexpr (TRAIN) {
    gp[0] = r;
    gp[hd] = z;
    gp[2 * hd] = n;
    gp[3 * hd] = hn;
  }
  return (1.0f - z) * n + z * hprev;
}

template <int DT, int NF, bool TRAIN>
__global__ __launch_bounds__(256) void k_half_gru(const float *__restrict__ a, int64_t ld_a,
                                                  const float *__restrict__ h, int64_t ld_h,
                                                  const uint16_t *__restrict__ w_ih, const uint16_t *__restrict__ w_hh,
                                                  const float *__restrict__ b_ih, const float *__restrict__ b_hh,
                                                  int64_t n, int M, int Hd, float *__restrict__ out, int64_t ld_out,
                                                  int col_groups, float *__restrict__ gates) {
  using H = Half16<DT>;
  const int wave = threadIdx.x >> 6, li = frag_li(), hi = frag_hi();
  const int64_t row0 = ((int64_t)(blockIdx.x / col_groups) * 4 + wave) * 32;
  if (row0 >= n) return;                         // no barrier in this kernel
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
    // not for_frag_rows: at NF = 2 this kernel sits at 160 + 96 registers, and the helper's 2 more halve its occupancy
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + frag_row(r, hi);
      if (row < n) {
        const float hprev = h[row * ld_h + j];    // the UNROUNDED state (L2-hot: phase 1 just streamed the row)
        out[row * ld_out + j] = gru_gate<TRAIN>(acc[f][0][r], acc[f][1][r], acc[f][2][r], acc[f][3][r], hprev, bir, biz,
                                                bin, bhr, bhz, bhn, TRAIN ? gates + row * 4 * Hd + j : nullptr, Hd);
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
//     of the launch workgroup-strided, each panel's [a | h] rows through a RoundedPanel (half16.h).
// Same chains as k_half_gru (k ascending, the a phase before the h phase, one accumulator per gate) and the same gate
// math: the two kernels give the same bits, so which one runs (a function of M and H alone) is not observable
// (tests/test_gpu_half_inputs.py holds one against the other).
// ---------------------------------------------------------------------------------------------
template <int DT, int KA, int KH, bool TRAIN>
__global__ __launch_bounds__(256) void k_half_gru_ws(const float *__restrict__ a, int64_t ld_a,
                                                     const float *__restrict__ h, int64_t ld_h,
                                                     const uint16_t *__restrict__ w_ih,
                                                     const uint16_t *__restrict__ w_hh,
                                                     const float *__restrict__ b_ih, const float *__restrict__ b_hh,
                                                     int64_t n, float *__restrict__ out, int64_t ld_out,
                                                     int64_t num_panels, float *__restrict__ gates) {
  using H = Half16<DT>;
  using vec = typename H::vec;
  constexpr int M = 16 * KA, Hd = 16 * KH, KS = KA + KH;
  constexpr int S = Hd / 32;             // feature slices = waves per row unit (2 or 4)
  constexpr int PR = 32 * (4 / S);       // rows per panel (64 or 32)
  RoundedPanel<DT, PR, M + Hd> panel;

  const int wave = threadIdx.x >> 6, li = frag_li(), hi = frag_hi();
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

  auto rows_of = [&](int64_t p) {        // panel p's [a | h] rows (rows past n: the last valid row)
    return [=](int r, int c) {
      int64_t row = p * PR + r;
      row = row < n ? row : n - 1;
      return c < M ? a + row * ld_a + c : h + row * ld_h + (c - M);
    };
  };

  int64_t p = blockIdx.x;
  if (p >= num_panels) return;           // whole workgroup: before any barrier
  panel.prime(rows_of(p));
  for (; p < num_panels; p += gridDim.x) {
    const int64_t next = p + gridDim.x;
    panel.fetch(rows_of(next < num_panels ? next : p));

    f32x16 acc[4];   // r, z, i_n, h_n
#pragma unroll
    for (int g = 0; g < 4; ++g) zero(acc[g]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const vec av = panel.frag(ru * 32 + li, ks);
      acc[0] = H::mfma(av, bw[0][ks], acc[0]);
      acc[1] = H::mfma(av, bw[1][ks], acc[1]);
      if (ks < KA) acc[2] = H::mfma(av, bw[2][ks], acc[2]);
      else         acc[3] = H::mfma(av, bw[2][ks], acc[3]);
    }
    for_frag_rows(p * PR + ru * 32, n, [&](int r, int64_t row) {
      const float hprev = h[row * ld_h + j];    // the UNROUNDED state
      out[row * ld_out + j] = gru_gate<TRAIN>(acc[0][r], acc[1][r], acc[2][r], acc[3][r], hprev, bir, biz, bin, bhr, bhz,
                                              bhn, TRAIN ? gates + row * 4 * Hd + j : nullptr, Hd);
    });
    panel.flip();
  }
}

bool shape_ok(int kind, int32_t k_or_m, int32_t n_out_or_hd) {
  if (kind == PTGNN_AMD_HALF_KIND_LINEAR)
    return k_or_m > 0 && k_or_m % 32 == 0 && k_or_m <= 1024 && n_out_or_hd > 0 && n_out_or_hd % 32 == 0;
  if (kind == PTGNN_AMD_HALF_KIND_GRU)
    return k_or_m > 0 && k_or_m % 32 == 0 && k_or_m <= 1024 && n_out_or_hd > 0 && n_out_or_hd % 32 == 0 &&
           n_out_or_hd <= 1024;
  if (kind == PTGNN_AMD_HALF_KIND_WGRAD)      // csrc/wgrad16.hip: k, n_out
    return k_or_m > 0 && k_or_m % 32 == 0 && k_or_m <= 1024 && n_out_or_hd > 0 && n_out_or_hd % 32 == 0 &&
           n_out_or_hd <= 1024;
  return false;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_half_supported(int kind, int32_t k_or_m, int32_t n_out_or_hd, int dtype) {
  return dtype_ok(dtype) && shape_ok(kind, k_or_m, n_out_or_hd) ? 1 : 0;
}

// the two Linear entries: `what` names the entry in the messages; ADD: with the fp32 addend
template <bool ADD>
static int half_linear_entry(const char *what, const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w,
                             int32_t n_out, const float *bias, int act, int dtype, const float *addend, int64_t ld_add,
                             float *y, int64_t ld_y, void *stream_) {
  PTGNN_REQUIRE(rows >= 0 && k > 0 && n_out > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(act >= 0 && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "%s: bad act", what);
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", what, dtype);
  PTGNN_REQUIRE(shape_ok(PTGNN_AMD_HALF_KIND_LINEAR, k, n_out), PTGNN_AMD_EUNSUPPORTED,
                "%s: k=%d n_out=%d: needs k %% 32 == 0, k <= 1024, n_out %% 32 == 0", what, k, n_out);
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && w && y && ld_x >= k && ld_y >= n_out, PTGNN_AMD_EINVAL, "%s: null/ld", what);
  PTGNN_REQUIRE(!ADD || (addend && ld_add >= n_out), PTGNN_AMD_EINVAL, "%s: null/ld of the addend", what);
  PTGNN_REQUIRE(rows16(x, ld_x) && aligned16(w) && aligned4(y) && (!bias || aligned4(bias)) &&
                    (!ADD || aligned4(addend)),
                PTGNN_AMD_EUNSUPPORTED,
                "%s: x and w must be 16-byte aligned with ld_x %% 4 == 0 (ld_x=%lld), y and bias float-aligned", what,
                (long long)ld_x);
  const int col_groups = (n_out + 32 * kLinTiles - 1) / (32 * kLinTiles);
  const int64_t blocks = (rows + 127) / 128 * col_groups;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many tiles", what);
  hipStream_t st = (hipStream_t)stream_;
  const uint16_t *w16 = static_cast<const uint16_t *>(w);
  with_dtype(dtype, [&](auto dt) {
    k_half_linear<decltype(dt)::value, ADD><<<(unsigned)blocks, 256, 0, st>>>(x, rows, k, ld_x, w16, n_out, bias, act, y,
                                                                              ld_y, col_groups, addend, ld_add);
  });
  PTGNN_LAUNCH_CHECK();
  count_launch(ADD ? PTGNN_AMD_KERNEL_HALF_LINEAR_ADD : PTGNN_AMD_KERNEL_HALF_LINEAR);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_half_linear(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w,
                                     int32_t n_out, const float *bias, int act, int dtype, float *y, int64_t ld_y,
                                     void *stream_) {
  return half_linear_entry<false>("half_linear", x, rows, k, ld_x, w, n_out, bias, act, dtype, nullptr, 0, y, ld_y,
                                  stream_);
}

extern "C" int ptgnn_amd_linear_add16(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w,
                                      int32_t n_out, const float *bias, int act, int dtype, const float *addend,
                                      int64_t ld_add, float *y, int64_t ld_y, void *stream_) {
  return half_linear_entry<true>("linear_add16", x, rows, k, ld_x, w, n_out, bias, act, dtype, addend, ld_add, y, ld_y,
                                 stream_);
}

// the two GRU entries: `what` names the entry in the messages; TRAIN: also writes gates [n, 4 hd]
template <bool TRAIN>
static int half_gru_entry(const char *what, const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                          const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m, int32_t hd,
                          int dtype, float *out, int64_t ld_out, float *gates, void *stream_) {
  PTGNN_REQUIRE(n >= 0 && m > 0 && hd > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", what, dtype);
  PTGNN_REQUIRE(shape_ok(PTGNN_AMD_HALF_KIND_GRU, m, hd), PTGNN_AMD_EUNSUPPORTED,
                "%s: m=%d hd=%d: needs m %% 32 == 0, hd %% 32 == 0, both <= 1024", what, m, hd);
  if (n == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(a && h && w_ih && w_hh && b_ih && b_hh && out && (!TRAIN || gates), PTGNN_AMD_EINVAL, "%s: null", what);
  PTGNN_REQUIRE(ld_a >= m && ld_h >= hd && ld_out >= hd, PTGNN_AMD_EINVAL, "%s: bad ld", what);
  PTGNN_REQUIRE(out != h, PTGNN_AMD_EINVAL, "%s: in-place update is not supported", what);
  PTGNN_REQUIRE(rows16(a, ld_a) && rows16(h, ld_h) && aligned16(w_ih) && aligned16(w_hh) && aligned4(out) &&
                    aligned4(b_ih) && aligned4(b_hh) && (!TRAIN || aligned4(gates)),
                PTGNN_AMD_EUNSUPPORTED,
                "%s: a, h and the weights must be 16-byte aligned with ld %% 4 == 0 (ld_a=%lld, ld_h=%lld), "
                "out and the biases float-aligned", what, (long long)ld_a, (long long)ld_h);
  const int nf = hd % 64 == 0 ? 2 : 1;
  const int col_groups = hd / (32 * nf);
  const int64_t blocks = (n + 127) / 128 * col_groups;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many tiles", what);
  hipStream_t st = (hipStream_t)stream_;
  const uint16_t *wi = static_cast<const uint16_t *>(w_ih), *wh = static_cast<const uint16_t *>(w_hh);
  const bool ws = (m == 64 || m == 128) && (hd == 64 || hd == 128);   // the GGNN widths: weight-stationary (same bits)
  const int64_t num_panels = (n + (hd == 128 ? 31 : 63)) / (hd == 128 ? 32 : 64);
  const int64_t cus = ws ? num_compute_units() : 0;
  const unsigned grid = (unsigned)(num_panels < cus ? num_panels : cus);
  with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (ws)
      with_case<4, 8>(m / 16, [&](auto ka) {
        with_case<4, 8>(hd / 16, [&](auto kh) {
          k_half_gru_ws<DT, decltype(ka)::value, decltype(kh)::value, TRAIN><<<grid, 256, 0, st>>>(
              a, ld_a, h, ld_h, wi, wh, b_ih, b_hh, n, out, ld_out, num_panels, gates);
        });
      });
    else
      with_case<1, 2>(nf, [&](auto f) {
        k_half_gru<DT, decltype(f)::value, TRAIN><<<(unsigned)blocks, 256, 0, st>>>(
            a, ld_a, h, ld_h, wi, wh, b_ih, b_hh, n, m, hd, out, ld_out, col_groups, gates);
      });
  });
  PTGNN_LAUNCH_CHECK();
  count_launch(TRAIN ? PTGNN_AMD_KERNEL_HALF_GRU_TRAIN : PTGNN_AMD_KERNEL_HALF_GRU);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_half_gru_cell(const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                                       const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m,
                                       int32_t hd, int dtype, float *out, int64_t ld_out, void *stream_) {
  return half_gru_entry<false>("half_gru_cell", a, ld_a, h, ld_h, w_ih, w_hh, b_ih, b_hh, n, m, hd, dtype, out, ld_out,
                               nullptr, stream_);
}

extern "C" int ptgnn_amd_gru_cell_train16(const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                                          const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m,
                                          int32_t hd, int dtype, float *out, int64_t ld_out, float *gates,
                                          void *stream_) {
  return half_gru_entry<true>("gru_cell_train16", a, ld_a, h, ld_h, w_ih, w_hh, b_ih, b_hh, n, m, hd, dtype, out, ld_out,
                              gates, stream_);
}
