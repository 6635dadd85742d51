// Opt-in 16-bit weight gradient of the GGNN layer's dense blocks: grad_w [n_out, k] = rnd(grad_y)^T rnd(x) on
// v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation; grad_b = column sums of the UNROUNDED fp32 grad_y.  Entry points
//   ptgnn_amd_linear_weight_grad16   : the product (and the bias gradient of the same pass)
//   ptgnn_amd_wgrad16_workspace_bytes: bytes of partials the call needs
//   ptgnn_amd_wgrad16_chunk_rows     : rows one workgroup partial covers; no device needed
// Contract: include/ptgnn_amd.h.  The MFMA, the rounded LDS panel and its transposed fragment: half16.h.
//
// The reduction index is the ROW index of both operands.  A workgroup (4 waves) owns a 128 x TN tile of grad_w
// (TN = 128, 64 or 32: the widest that divides k) over `chunk_rows` consecutive rows.  It walks them in panels of 32
// rows: the panel's [grad_y columns of the tile | x columns of the tile] are loaded ONCE as fp32, coalesced (a thread's
// float4s are consecutive in a row), rounded and parked in the 16-bit image of half16::RoundedPanel -- two buffers, the
// next panel's loads in flight under this panel's MFMAs, one barrier per panel -- and BOTH operands' fragments are read
// transposed (RoundedPanel::frag_tr: ds_read_b64_tr_b16).  No per-lane strided global load anywhere.
//
// LDS image: row stride LD = TM + TN elements when that is 32 x odd, else 32 more (288, 224, 160 elements for
// TN = 128, 64, 32: 576, 448, 320 bytes = 64 x {9, 7, 5}).  Bank conflicts, from the section 2 rule of
// cdna_hip_programming.md ((a / 4) % 64 per 32-lane half): a half's transposed read takes 4 consecutive rows x 64
// contiguous bytes; 64 x odd bytes between rows put the four 16-bank runs at banks {0, 16, 32, 48} + const: 64
// distinct banks, ZERO conflicts, for every TN.  The park's ds_write_b64 are contiguous 8-byte pieces of a row in
// lane order (a 32-lane group covers 256 contiguous bytes, broken only where a row ends): the minimum two passes.
//
// Rows past the end of a chunk are zeros in the image (they add nothing), never masked lanes; column sub-tiles of the
// 128 past n_out re-read a live sub-tile and are not stored: every lane runs every transposed read with EXEC all ones,
// and there is no `return` in the kernel.
//
// Determinism: every workgroup writes ONE fp32 partial tile (and, at the first column tile, one partial of the bias
// gradient) to the workspace; k_wgrad16_reduce adds the partials in a fixed order -- eight lanes per output float4, each
// over chunks sub, sub + 8, ... ascending, then a fixed xor butterfly (the scheme of edge_wgrad.hip's k_wgrad_reduce,
// whose kernel is tied to the fp32 tile's fragment order and so is not reused).  One chunk: the tile goes straight to
// grad_w.  No atomics, no inline assembly; every store is a plain C++ assignment.
//
// Partials.  chunk_rows = max(512, rows x tiles / 512 rounded up to 32): about 512 workgroups (two per CU), and per
// workgroup at most 2 x 128 x TN x 4 bytes of partial traffic (written, read once) against chunk_rows x (128 + TN) x 4
// bytes of operand rows: at most 1/4 at the 512-row floor and TN = 128, falling with 1 / chunk_rows.
#include "half16.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

constexpr int kTM = 128;          // grad_y columns (rows of grad_w) per workgroup tile
constexpr int kPE = 32;           // rows per panel: two MFMA k-steps
constexpr int kMinChunk = 512;    // rows
constexpr int kTargetGroups = 512;
constexpr int kSplit = 8;         // lanes per output float4 in the reduction

inline int tile_n(int k) { return k % 128 == 0 ? 128 : (k % 64 == 0 ? 64 : 32); }
inline int64_t tiles_of(int n_out, int k) { return (int64_t)((n_out + kTM - 1) / kTM) * (k / tile_n(k)); }

inline int64_t chunk_rows_for(int64_t rows, int n_out, int k) {
  const int64_t want = (rows * tiles_of(n_out, k) + kTargetGroups - 1) / kTargetGroups;
  const int64_t c = (want + kPE - 1) / kPE * kPE;
  return c > kMinChunk ? c : kMinChunk;
}
inline int64_t chunks_for(int64_t rows, int n_out, int k) {
  const int64_t c = chunk_rows_for(rows, n_out, k);
  return (rows + c - 1) / c;
}
// floats of one chunk's partial: the tile rows of grad_w, then the bias partial
inline int64_t partial_floats(int n_out, int k) { return (int64_t)n_out * k + n_out; }

template <int DT, int TN>
__global__ __launch_bounds__(256) void k_wgrad16(const float *__restrict__ x, int64_t ld_x, int K,
                                                 const float *__restrict__ g, int64_t ld_g, int64_t rows, int n_out,
                                                 int64_t chunk_rows, int jtiles, int tiles, float *__restrict__ out_w,
                                                 float *__restrict__ out_b, int64_t out_stride) {
  using H = Half16<DT>;
  using vec = typename H::vec;
  constexpr int KT = kTM + TN;
  constexpr int LD = (KT / 32) % 2 == 1 ? KT : KT + 32;
  using Panel = RoundedPanel<DT, kPE, KT, LD>;
  constexpr int NJ = TN / 32, WJ = NJ >= 2 ? 2 : 1, WM = 4 / WJ, SM = 4 / WM, SJ = NJ / WJ;
  static_assert(kPE * kTM * 4 <= 2 * kPE * LD * 2, "the bias scratch reuses the panel buffers");
  Panel panel;

  const int wave = threadIdx.x >> 6, li = frag_li();
  const int wm = wave / WJ, wn = wave % WJ;
  const int tile = (int)(blockIdx.x % tiles);
  const int64_t chunk = blockIdx.x / tiles;
  const int m0 = (tile / jtiles) * kTM, j0 = (tile % jtiles) * TN;
  const int64_t e0 = chunk * chunk_rows;
  const int64_t e1 = e0 + chunk_rows < rows ? e0 + chunk_rows : rows;     // e1 > e0: the grid has no empty chunk
  const int64_t num_panels = (e1 - e0 + kPE - 1) / kPE;
  const bool with_bias = out_b != nullptr && j0 == 0;                    // workgroup-uniform

  auto rows_of = [&](int64_t p) {        // panel p: [grad_y columns m0 .. | x columns j0 ..] of rows e0 + 32 p ..
    return [=](int r, int c) {
      const int64_t row = e0 + p * kPE + r;                               // < e1 wherever fetch dereferences
      const int gc = m0 + c < n_out ? m0 + c : m0 + c % 32;               // a sub-tile past n_out: a live one, not stored
      return c < kTM ? g + row * ld_g + gc : x + row * ld_x + j0 + (c - kTM);
    };
  };
  auto live_of = [&](int64_t p) {
    const int64_t left = e1 - (e0 + p * kPE);
    return (int)(left < kPE ? (left > 0 ? left : 0) : kPE);
  };

  f32x16 acc[SM][SJ];
#pragma unroll
  for (int a = 0; a < SM; ++a)
#pragma unroll
    for (int b = 0; b < SJ; ++b) zero(acc[a][b]);
  float4 bsum[Panel::NV];                // this thread's fp32 column sums: slot i is the same (row, columns) every panel
#pragma unroll
  for (int i = 0; i < Panel::NV; ++i) bsum[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add_bias = [&]() {
    if (with_bias) {
#pragma unroll
      for (int i = 0; i < Panel::NV; ++i) {
        bsum[i].x += panel.stage[i].x; bsum[i].y += panel.stage[i].y;
        bsum[i].z += panel.stage[i].z; bsum[i].w += panel.stage[i].w;
      }
    }
  };

  panel.prime(rows_of(0), live_of(0));
  add_bias();
  for (int64_t p = 0; p < num_panels; ++p) {
    panel.fetch(rows_of(p + 1), live_of(p + 1));        // past the last panel: live = 0, zeros, no load
#pragma unroll
    for (int ks = 0; ks < kPE / 16; ++ks) {
      vec av[SM], bv[SJ];
#pragma unroll
      for (int a = 0; a < SM; ++a) av[a] = panel.frag_tr(16 * ks, (wm * SM + a) * 32);
#pragma unroll
      for (int b = 0; b < SJ; ++b) bv[b] = panel.frag_tr(16 * ks, kTM + (wn * SJ + b) * 32);
#pragma unroll
      for (int a = 0; a < SM; ++a)
#pragma unroll
        for (int b = 0; b < SJ; ++b) acc[a][b] = H::mfma(av[a], bv[b], acc[a][b]);
    }
    panel.flip();
    add_bias();
  }

  // the partial tile: register r of sub-tile (a, b) is grad_w[m0 + 32 (wm SM + a) + frag_row(r)][j0 + 32 (wn SJ + b) + li]
  float *pw = out_w + chunk * out_stride;
#pragma unroll
  for (int a = 0; a < SM; ++a) {
    const int ms = m0 + (wm * SM + a) * 32;
    if (ms < n_out) {                                   // wave-uniform; no transposed read follows
#pragma unroll
      for (int b = 0; b < SJ; ++b) {
        const int j = j0 + (wn * SJ + b) * 32 + li;
        for_frag_rows(ms, n_out, [&](int r, int64_t m) { pw[m * K + j] = acc[a][b][r]; });
      }
    }
  }

  if (with_bias) {   // 32 row-partials per column meet in LDS (the last flip's barrier: nobody reads the panels any more)
    float *scratch = reinterpret_cast<float *>(Panel::buffer(0));
#pragma unroll
    for (int i = 0; i < Panel::NV; ++i) {
      const int v = threadIdx.x + i * 256, r = v / Panel::RV, c = (v % Panel::RV) * 4;
      if (c < kTM) *reinterpret_cast<float4 *>(scratch + r * kTM + c) = bsum[i];
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < kTM && m0 + c < n_out) {
      float s = 0.f;
      for (int r = 0; r < kPE; ++r) s += scratch[r * kTM + c];
      (out_b + chunk * out_stride)[m0 + c] = s;
    }
  }
}

// out[f] = sum over chunks of partial[chunk][f], f a float4 of [grad_w | grad_b]: fixed order (file header)
__global__ __launch_bounds__(256) void k_wgrad16_reduce(const float *__restrict__ partial, int64_t chunks,
                                                        int64_t stride, int64_t w4, int64_t total4,
                                                        float *__restrict__ grad_w, float *__restrict__ grad_b) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t f = gid / kSplit;
  const int sub = (int)(gid % kSplit);
  if (f >= total4) return;                             // whole 8-lane groups leave together
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t c = sub; c < chunks; c += kSplit) {
    const float4 p = *reinterpret_cast<const float4 *>(partial + c * stride + f * 4);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
#pragma unroll
  for (int d = 1; d < kSplit; d <<= 1) {
    s.x += __shfl_xor(s.x, d); s.y += __shfl_xor(s.y, d);
    s.z += __shfl_xor(s.z, d); s.w += __shfl_xor(s.w, d);
  }
  if (sub == 0) *reinterpret_cast<float4 *>(f < w4 ? grad_w + f * 4 : grad_b + (f - w4) * 4) = s;
}

bool wgrad_shape_ok(int32_t k, int32_t n_out) {
  return k > 0 && k % 32 == 0 && k <= 1024 && n_out > 0 && n_out % 32 == 0 && n_out <= 1024;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int64_t ptgnn_amd_wgrad16_chunk_rows(int64_t rows, int32_t n_out, int32_t k) {
  if (rows < 0 || !wgrad_shape_ok(k, n_out)) return 0;
  return chunk_rows_for(rows, n_out, k);
}

extern "C" size_t ptgnn_amd_wgrad16_workspace_bytes(int64_t rows, int32_t n_out, int32_t k) {
  if (rows <= 0 || !wgrad_shape_ok(k, n_out)) return 0;
  const int64_t chunks = chunks_for(rows, n_out, k);
  return chunks <= 1 ? 0 : (size_t)chunks * (size_t)partial_floats(n_out, k) * sizeof(float);
}

extern "C" int ptgnn_amd_linear_weight_grad16(const float *x, int64_t ld_x, int32_t k, const float *grad_y,
                                              int64_t ld_grad_y, int64_t rows, int32_t n_out, int dtype,
                                              float *grad_w, float *grad_b, void *workspace, size_t workspace_bytes,
                                              void *stream_) {
  PTGNN_REQUIRE(rows >= 0 && k > 0 && n_out > 0, PTGNN_AMD_EINVAL, "linear_weight_grad16: bad sizes");
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL,
                "linear_weight_grad16: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16", dtype);
  PTGNN_REQUIRE(wgrad_shape_ok(k, n_out), PTGNN_AMD_EUNSUPPORTED,
                "linear_weight_grad16: k=%d n_out=%d: needs k %% 32 == 0, n_out %% 32 == 0, both <= 1024", k, n_out);
  PTGNN_REQUIRE(grad_w, PTGNN_AMD_EINVAL, "linear_weight_grad16: null");
  PTGNN_REQUIRE(aligned16(grad_w) && (!grad_b || aligned16(grad_b)), PTGNN_AMD_EUNSUPPORTED,
                "linear_weight_grad16: grad_w and grad_b must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream_;
  if (rows == 0) {   // zeros, no launch
    PTGNN_HIP(hipMemsetAsync(grad_w, 0, (size_t)n_out * k * sizeof(float), st));
    if (grad_b) PTGNN_HIP(hipMemsetAsync(grad_b, 0, (size_t)n_out * sizeof(float), st));
    return PTGNN_AMD_OK;
  }
  PTGNN_REQUIRE(x && grad_y && ld_x >= k && ld_grad_y >= n_out, PTGNN_AMD_EINVAL, "linear_weight_grad16: null/ld");
  PTGNN_REQUIRE(rows16(x, ld_x) && rows16(grad_y, ld_grad_y), PTGNN_AMD_EUNSUPPORTED,
                "linear_weight_grad16: x and grad_y must be 16-byte aligned with ld %% 4 == 0 (ld_x=%lld, "
                "ld_grad_y=%lld)", (long long)ld_x, (long long)ld_grad_y);
  const int64_t chunk = chunk_rows_for(rows, n_out, k), chunks = chunks_for(rows, n_out, k);
  const int tn = tile_n(k), jtiles = k / tn;
  const int64_t tiles = tiles_of(n_out, k), blocks = tiles * chunks;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "linear_weight_grad16: too many tiles");
  const size_t need = ptgnn_amd_wgrad16_workspace_bytes(rows, n_out, k);
  PTGNN_REQUIRE(workspace_bytes >= need && (need == 0 || (workspace && aligned16(workspace))), PTGNN_AMD_EINVAL,
                "linear_weight_grad16: workspace too small or unaligned (%zu bytes, needs %zu)", workspace_bytes, need);
  const bool direct = chunks == 1;
  const int64_t stride = partial_floats(n_out, k);
  float *out_w = direct ? grad_w : static_cast<float *>(workspace);
  float *out_b = !grad_b ? nullptr : (direct ? grad_b : out_w + (int64_t)n_out * k);
  with_dtype(dtype, [&](auto dt) {
    with_case<128, 64, 32>(tn, [&](auto t) {
      k_wgrad16<decltype(dt)::value, decltype(t)::value><<<(unsigned)blocks, 256, 0, st>>>(
          x, ld_x, k, grad_y, ld_grad_y, rows, n_out, chunk, jtiles, (int)tiles, out_w, out_b, stride);
    });
  });
  PTGNN_LAUNCH_CHECK();
  if (!direct) {
    const int64_t w4 = (int64_t)n_out * k / 4, total4 = w4 + (grad_b ? n_out / 4 : 0);
    k_wgrad16_reduce<<<(unsigned)((total4 * kSplit + 255) / 256), 256, 0, st>>>(out_w, chunks, stride, w4, total4,
                                                                               grad_w, grad_b);
    PTGNN_LAUNCH_CHECK();
  }
  count_launch(PTGNN_AMD_KERNEL_HALF_WGRAD);
  return PTGNN_AMD_OK;
}
