// Opt-in panel-form 16-bit Linear of the attention layer's TRAINING step: 16-bit (bf16 / fp16) operands on the matrix
// cores (v_mfma_f32_32x32x16_{bf16,f16}), BOTH operands staged through LDS, Dropout(act(.)) and the residual add in the
// store epilogue, and the masked input gradient of the same node.  The C-ABI entry points
//   ptgnn_amd_panel_linear16            : y = dropout_p(act(rnd(x) rnd(W)^T + b)) + addend   (y_act: the value before dropout)
//   ptgnn_amd_panel_linear16_grad_input : d_x = rnd(g * (keep ? scale : 0) * act'(y)) rnd(W)
//   ptgnn_amd_panel_linear16_supported  : the shape check of the two, no device needed
// (the masked weight gradient of the node is a mode of csrc/wgrad16.hip).  Contracts: include/ptgnn_amd.h.  The MFMA, the
// chain and the rounded LDS panel: half16.h.
//
// Why a second 16-bit Linear.  k_half_linear (half_gemm.hip) loads every A fragment from global memory one ROW per lane
// (64 cache lines per load instruction) and re-reads the weights from L2 per wave: one global fragment load per MFMA.
// At the attention layer's widths (256 -> 256 -> 1024 -> 256 over 1e5 rows) the GEMMs are bound by the matrix rate, and
// that kernel is level with exact fp32.  Here one workgroup (256 threads) owns 128 rows x 128 output columns; per panel
// of KT reduction columns
//   * the A panel (128 rows x KT fp32) is loaded ONCE, coalesced as float4, rounded and parked as a 16-bit image
//     (half16::RoundedPanel: two buffers, the next panel's loads issued before this panel's MFMAs and parked after
//     them, one barrier per panel);
//   * the B panel (the same KT columns of the tile's 128 weight rows, already 16-bit) is copied into LDS as dwordx4 by
//     WeightPanel below, at the same row stride (KT + 8 elements: an odd number of 16-byte units -> conflict-free
//     ds_read_b128, the rule of half16.h);
//   * the four waves are laid out 2 x 2, each owning 64 x 64 = 2 x 2 accumulators: per k-step two A and two B fragment
//     reads from LDS feed four MFMAs.
// The grid puts the column tile fastest, so the workgroups sharing an A row tile are co-resident: x comes from HBM once.
//
// The chain is the one of every 16-bit kernel here: an output element is ONE fp32 accumulator, zeroed, k ascending in
// steps of 16 over operands rounded to nearest even -- so row r's bits do not depend on the row count, the tile position
// or KT, and with p = 0 and no addend they are ptgnn_amd_half_linear's.  Panel columns past K are zeros in BOTH images
// (K % 32 == 0 only; at KT = 64 the last panel may be half empty); rows past `rows` read a clamped valid row and are
// never stored; column sub-tiles past n_out re-read a live sub-tile and are not stored.  No masked lanes before the
// epilogue, no `return` before the last barrier.
//
// KT is a template constant: 32 (stride 40, 40 960 bytes of LDS: three workgroups per CU) or 64 (stride 72, 73 728
// bytes: two per CU, needs the dynamic-LDS opt-in).  The B image is the dynamic part of the allocation either way.
// Which one runs: kForwardKT / kGradKT below, measured in profiles/attention_linears_notes.md.
//
// No atomics, no inline assembly; every store is a plain C++ assignment.
#include <cstdlib>

#include "half16.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

constexpr int kTile = 128;        // rows and output columns of a workgroup tile
// the panel width the entries launch, as measured (profiles/attention_linears_notes.md): the forward is faster at 64,
// the input gradient (whose edit holds the staged panel longer) at 32; PTGNN_AMD_PANEL16_KT=32|64 overrides both, for
// the benchmark leg
constexpr int kForwardKT = 64, kGradKT = 32;
constexpr int kMaxWidth = 4096;

enum { MODE_FWD = 0, MODE_FWD_ADD = 1, MODE_GRAD = 2, MODE_GRAD_ACT = 3 };

// The 16-bit-source sibling of RoundedPanel: ROWS = 128 rows x KT already-rounded 16-bit values per buffer, staged through
// registers as dwordx4 (8 elements) and parked at RoundedPanel's row stride.  src(r, c): the address of the 8 elements at
// row r, columns c .. c + 7 of a panel; panel columns >= `kleft` are zeros in the image and are not loaded.
template <int DT, int KT>
struct WeightPanel {
  using vec = typename Half16<DT>::vec;
  static constexpr int LD = KT + 8;
  static constexpr int RV = KT / 8;              // dwordx4 per panel row
  static constexpr int NV = kTile * RV / 256;    // dwordx4 per thread and panel
  static_assert(kTile * RV % 256 == 0, "panel shape");

  uint4 stage[NV];

  template <class Src>
  __device__ __forceinline__ void fetch(Src &&src, int kleft) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256, c = (v % RV) * 8;
      stage[i] = c < kleft ? *reinterpret_cast<const uint4 *>(src(v / RV, c)) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __device__ __forceinline__ void park(uint16_t *buf) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = threadIdx.x + i * 256;
      *reinterpret_cast<uint4 *>(buf + (v / RV) * LD + (v % RV) * 8) = stage[i];
    }
  }
  // this lane's B fragment of k-step ks in row `row` (an output column of the tile) of the image at `buf`
  static __device__ __forceinline__ vec frag(const uint16_t *buf, int row, int ks) {
    return *reinterpret_cast<const vec *>(buf + row * LD + ks * 16 + 8 * frag_hi());
  }
};

struct PanelArgs {
  const float *a;        // [rows, K] fp32: x (forward) or grad_y (input gradient)
  int64_t ld_a;
  int64_t rows;
  int K;                 // reduction width: k (forward), n_out (input gradient)
  const uint16_t *w;     // [N, K] rounded: W (forward), W^T (input gradient)
  int N;                 // output width
  float *out;
  int64_t ld_out;
  int col_tiles;
  int act;
  DropoutParams drop;    // half_width = (forward n_out) / 2; thr == 0: no dropout
  // forward
  const float *bias;     // nullable
  const float *addend;   // MODE_FWD_ADD
  int64_t ld_add;
  float *y_act;          // nullable
  int64_t ld_y_act;
  // input gradient
  const float *y;        // MODE_GRAD_ACT: the activation's output rows [rows, K]
  int64_t ld_y;
};

// The forward epilogue of one 32 x 32 sub-tile (first row ms, this lane's column `col`): every operation fp32 and
// individually rounded, in the order of include/ptgnn_amd.h.
template <bool ADD>
__device__ __forceinline__ void store_forward(const PanelArgs &p, const f32x16 &acc, int64_t ms, int col) {
#pragma clang fp contract(off)
  const int hi = frag_hi();
  const float bv = p.bias ? p.bias[col] : 0.f;
  float av[16];
  if constexpr (ADD) {   // the sub-tile's 16 addends in flight together (rows past the end: the last row, never stored)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = ms + frag_row(r, hi);
      av[r] = p.addend[(row < p.rows ? row : p.rows - 1) * p.ld_add + col];
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = ms + frag_row(r, hi);
    if (row < p.rows) {
      float v = act_runtime(acc[r] + bv, p.act);
      if (p.y_act) p.y_act[row * p.ld_y_act + col] = v;
      if (p.drop.thr != 0) {
        const uint32_t bits = dropout_bits(p.drop, row, col >> 1);
        const uint32_t mine = (col & 1) ? bits >> 16 : bits & 0xffffu;
        v = mine >= p.drop.thr ? v * p.drop.scale : 0.f;
      }
      if constexpr (ADD) v = v + av[r];
      p.out[row * p.ld_out + col] = v;
    }
  }
}

// Two workgroups per CU (the second launch bound): without it the forward epilogue's hoisted row addresses take the
// kernel past 256 registers and down to one wave per SIMD; a third (KT = 32's LDS would allow it) costs scratch.
template <int DT, int MODE, int KT>
__global__ __launch_bounds__(256, 2) void k_panel_linear16(PanelArgs p) {
  using H = Half16<DT>;
  using vec = typename H::vec;
  using APanel = RoundedPanel<DT, kTile, KT>;
  using BPanel = WeightPanel<DT, KT>;
  constexpr bool GRAD = MODE == MODE_GRAD || MODE == MODE_GRAD_ACT;
  constexpr bool EDIT = GRAD || KT > 32;          // the staged A panel is touched before its rounding
  extern __shared__ __attribute__((aligned(16))) uint16_t wimage[];   // [2][kTile * BPanel::LD]
  APanel ap;
  BPanel bp;

  const int wave = threadIdx.x >> 6, li = frag_li();
  const int wr = wave >> 1, wc = wave & 1;
  const int col0 = (int)(blockIdx.x % p.col_tiles) * kTile;
  const int64_t row0 = (int64_t)(blockIdx.x / p.col_tiles) * kTile;
  const int K = p.K, N = p.N;
  const int64_t rows = p.rows;
  const int num_panels = (K + KT - 1) / KT;

  auto clamp_row = [&](int r) {
    const int64_t row = row0 + r;
    return row < rows ? row : rows - 1;           // rows past the end read the last valid row, never stored
  };
  auto a_src = [&](const float *base, int64_t ld, int k0) {
    return [=](int r, int c) {
      const int64_t row = row0 + r < rows ? row0 + r : rows - 1;
      const int kc = KT > 32 && k0 + c >= K ? 0 : k0 + c;   // past K: any valid address; the edit zeroes the values
      return base + row * ld + kc;
    };
  };
  auto b_src = [&](int k0) {
    return [=](int r, int c) {
      const int col = col0 + r < N ? col0 + r : col0 + r % 32;   // a sub-tile past n_out: a live one, not stored
      return p.w + (int64_t)col * K + k0 + c;
    };
  };
  float4 ys[MODE == MODE_GRAD_ACT ? APanel::NV : 1];
  auto fetch = [&](int pn) {
    const int k0 = pn * KT;
    ap.fetch(a_src(p.a, p.ld_a, k0));
    if constexpr (MODE == MODE_GRAD_ACT) {
      auto ysrc = a_src(p.y, p.ld_y, k0);
#pragma unroll
      for (int i = 0; i < APanel::NV; ++i) {
        const int v = threadIdx.x + i * 256;
        ys[i] = *reinterpret_cast<const float4 *>(ysrc(v / APanel::RV, (v % APanel::RV) * 4));
      }
    }
    bp.fetch(b_src(k0), K - k0);
  };
  // on the panel last fetched, before its one rounding: zeros past K; the masked gradient g' (half16.h masked_grad4)
  auto edit = [&](int pn) {
    if constexpr (EDIT) {
      const int k0 = pn * KT;
      ap.edit([&](int i, int r, int c, float4 &v) {
        if (KT > 32 && k0 + c >= K) {
          v = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if constexpr (GRAD) {
          v = masked_grad4<MODE == MODE_GRAD_ACT>(v, MODE == MODE_GRAD_ACT ? ys[i] : v, p.act, p.drop, clamp_row(r),
                                                  k0 + c);
        }
      });
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) zero(acc[a][b]);

  fetch(0);
  edit(0);
  bp.park(wimage);
  ap.start();
  for (int pn = 0; pn < num_panels; ++pn) {
    const int next = pn + 1 < num_panels ? pn + 1 : pn;   // the last trip re-fetches its own panel: no branch around loads
    fetch(next);
    const uint16_t *bcur = wimage + ap.cur * (kTile * BPanel::LD);
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
      vec av[2], bv[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) av[a] = ap.frag(wr * 64 + a * 32 + li, ks);
#pragma unroll
      for (int b = 0; b < 2; ++b) bv[b] = BPanel::frag(bcur, wc * 64 + b * 32 + li, ks);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = H::mfma(av[a], bv[b], acc[a][b]);
    }
    edit(next);
    bp.park(wimage + (ap.cur ^ 1) * (kTile * BPanel::LD));
    ap.flip();
  }

#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int64_t ms = row0 + wr * 64 + a * 32;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int cs = col0 + wc * 64 + b * 32;
      if (cs < N && ms < rows) {                          // wave-uniform
        const int col = cs + li;
        if constexpr (GRAD) for_frag_rows(ms, rows, [&](int r, int64_t row) { p.out[row * p.ld_out + col] = acc[a][b][r]; });
        else store_forward<MODE == MODE_FWD_ADD>(p, acc[a][b], ms, col);
      }
    }
  }
}

bool panel_shape_ok(int32_t k, int32_t n_out) {
  return k > 0 && k % 32 == 0 && k <= kMaxWidth && n_out > 0 && n_out % 32 == 0 && n_out <= kMaxWidth;
}

int panel_kt(bool grad) {   // the measured width, or the override the benchmark leg uses to measure the other one
  static const int forced = [] {
    const char *e = getenv("PTGNN_AMD_PANEL16_KT");
    const int v = e ? atoi(e) : 0;
    return v == 32 || v == 64 ? v : 0;
  }();
  return forced ? forced : (grad ? kGradKT : kForwardKT);
}

// one launch of mode MODE; KT = 64 needs more than 64 KiB of LDS: where the runtime refuses it, KT = 32 (same bits)
template <int MODE>
int launch_panel(const char *what, const PanelArgs &p, int dtype, hipStream_t st) {
  const int64_t blocks = (p.rows + kTile - 1) / kTile * p.col_tiles;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many tiles", what);
  bool wide = panel_kt(MODE == MODE_GRAD || MODE == MODE_GRAD_ACT) == 64;
  with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    constexpr size_t lds64 = (size_t)2 * kTile * WeightPanel<DT, 64>::LD * 2, lds32 = (size_t)2 * kTile * WeightPanel<DT, 32>::LD * 2;
    constexpr size_t total64 = 2 * lds64;                 // with RoundedPanel's static image
    auto k64 = k_panel_linear16<DT, MODE, 64>;
    if (wide && !raise_dynamic_lds(k64, total64)) wide = false;
    if (wide) k64<<<(unsigned)blocks, 256, lds64, st>>>(p);
    else k_panel_linear16<DT, MODE, 32><<<(unsigned)blocks, 256, lds32, st>>>(p);
  });
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_panel_linear16_supported(int32_t k, int32_t n_out, int dtype) {
  return dtype_ok(dtype) && panel_shape_ok(k, n_out) ? 1 : 0;
}

extern "C" int ptgnn_amd_panel_linear16(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w,
                                        int32_t n_out, const float *bias, int act, float p, uint64_t seed, int dtype,
                                        const float *addend, int64_t ld_add, float *y_act, int64_t ld_y_act, float *y,
                                        int64_t ld_y, void *stream_) {
  const char *what = "panel_linear16";
  PTGNN_REQUIRE(rows >= 0 && k > 0 && n_out > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(act >= PTGNN_AMD_ACT_NONE && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "%s: bad act", what);
  PTGNN_REQUIRE(p >= 0.f && p < 1.f, PTGNN_AMD_EINVAL, "%s: p must be in [0, 1)", what);
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", what, dtype);
  PTGNN_REQUIRE(panel_shape_ok(k, n_out), PTGNN_AMD_EUNSUPPORTED,
                "%s: k=%d n_out=%d: needs k %% 32 == 0, n_out %% 32 == 0, both <= %d", what, k, n_out, kMaxWidth);
  if (rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && w && y && ld_x >= k && ld_y >= n_out, PTGNN_AMD_EINVAL, "%s: null/ld", what);
  PTGNN_REQUIRE((!addend || ld_add >= n_out) && (!y_act || ld_y_act >= n_out), PTGNN_AMD_EINVAL,
                "%s: bad ld of the addend or y_act", what);
  PTGNN_REQUIRE(rows16(x, ld_x) && aligned16(w) && (!addend || rows16(addend, ld_add)), PTGNN_AMD_EUNSUPPORTED,
                "%s: x, w and the addend must be 16-byte aligned with ld %% 4 == 0 (ld_x=%lld, ld_add=%lld)", what,
                (long long)ld_x, (long long)ld_add);
  PTGNN_REQUIRE(aligned4(y) && (!bias || aligned4(bias)) && (!y_act || aligned4(y_act)), PTGNN_AMD_EUNSUPPORTED,
                "%s: y, y_act and bias must be float-aligned", what);
  PanelArgs a{};
  a.a = x; a.ld_a = ld_x; a.rows = rows; a.K = k;
  a.w = static_cast<const uint16_t *>(w); a.N = n_out;
  a.out = y; a.ld_out = ld_y;
  a.col_tiles = (n_out + kTile - 1) / kTile;
  a.act = act;
  a.drop = make_dropout(p, seed, n_out);
  a.bias = bias; a.addend = addend; a.ld_add = ld_add; a.y_act = y_act; a.ld_y_act = ld_y_act;
  hipStream_t st = (hipStream_t)stream_;
  const int rc = addend ? launch_panel<MODE_FWD_ADD>(what, a, dtype, st) : launch_panel<MODE_FWD>(what, a, dtype, st);
  if (rc != PTGNN_AMD_OK) return rc;
  count_launch(PTGNN_AMD_KERNEL_PANEL_LINEAR16);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_panel_linear16_grad_input(const float *grad_y, int64_t ld_grad_y, const float *y, int64_t ld_y,
                                                   int64_t rows, int32_t n_out, const void *wt, int32_t k, int act,
                                                   float p, uint64_t seed, int dtype, float *d_x, int64_t ld_dx,
                                                   void *stream_) {
  const char *what = "panel_linear16_grad_input";
  PTGNN_REQUIRE(rows >= 0 && k > 0 && n_out > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(act >= PTGNN_AMD_ACT_NONE && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "%s: bad act", what);
  PTGNN_REQUIRE(p >= 0.f && p < 1.f, PTGNN_AMD_EINVAL, "%s: p must be in [0, 1)", what);
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", what, dtype);
  PTGNN_REQUIRE(panel_shape_ok(k, n_out), PTGNN_AMD_EUNSUPPORTED,
                "%s: k=%d n_out=%d: needs k %% 32 == 0, n_out %% 32 == 0, both <= %d", what, k, n_out, kMaxWidth);
  if (rows == 0) return PTGNN_AMD_OK;
  const bool with_y = act != PTGNN_AMD_ACT_NONE;
  PTGNN_REQUIRE(grad_y && wt && d_x && ld_grad_y >= n_out && ld_dx >= k && (!with_y || (y && ld_y >= n_out)),
                PTGNN_AMD_EINVAL, "%s: null/ld (an activation needs its output rows y)", what);
  PTGNN_REQUIRE(rows16(grad_y, ld_grad_y) && aligned16(wt) && (!with_y || rows16(y, ld_y)) && aligned4(d_x),
                PTGNN_AMD_EUNSUPPORTED,
                "%s: grad_y, y and wt must be 16-byte aligned with ld %% 4 == 0 (ld_grad_y=%lld, ld_y=%lld), d_x "
                "float-aligned", what, (long long)ld_grad_y, (long long)ld_y);
  PanelArgs a{};
  a.a = grad_y; a.ld_a = ld_grad_y; a.rows = rows; a.K = n_out;
  a.w = static_cast<const uint16_t *>(wt); a.N = k;
  a.out = d_x; a.ld_out = ld_dx;
  a.col_tiles = (k + kTile - 1) / kTile;
  a.act = act;
  a.drop = make_dropout(p, seed, n_out);
  a.y = y; a.ld_y = ld_y;
  hipStream_t st = (hipStream_t)stream_;
  const int rc = with_y ? launch_panel<MODE_GRAD_ACT>(what, a, dtype, st) : launch_panel<MODE_GRAD>(what, a, dtype, st);
  if (rc != PTGNN_AMD_OK) return rc;
  count_launch(PTGNN_AMD_KERNEL_PANEL_LINEAR16_GRAD_INPUT);
  return PTGNN_AMD_OK;
}
