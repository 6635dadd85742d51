// Opt-in 16-bit weight gradient of the GGNN layer's per-edge message Linear, every edge type in one launch
// (the autograd of `edge_transformation_layer(...)` in gatedmessagepassing.py:57-61 under autocast):
//
//     grad_w[t] [M, H] = rnd(g_t)^T . rnd(keep ? x[src_t[e]] * scale : 0)      summed over the edges e of type t
//
// on v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation; g_t = the type's rows of grad_msg.  Entry points
//   ptgnn_amd_edge_weight_grad16          : the product
//   ptgnn_amd_edge_wgrad16_workspace_bytes: bytes of partials the call needs
//   ptgnn_amd_edge_wgrad16_chunk_edges    : edges one workgroup partial covers; no device needed
//   ptgnn_amd_edge_weight_grad16_supported: the shapes
// Contract: include/ptgnn_amd.h.  The MFMA, the rounded LDS panel and its transposed fragment: half16.h.
//
// The kernel is wgrad16.hip's with the chunk table of edge_wgrad.hip.  The reduction index is the EDGE of one type.  A
// workgroup (4 waves) owns a 128 x TN tile of one type's grad_w (TN = 128, 64 or 32: the widest that divides H) over one
// chunk of `chunk_edges` consecutive edges of that type -- the `chunk_off` prefix says which; a chunk never crosses a
// type.  It walks them in panels of 32 edges: the panel's [grad_msg columns of the tile | gathered x columns of the tile]
// are loaded ONCE as fp32 (a thread's float4s are consecutive in a row), rounded and parked in the 16-bit image of
// half16::RoundedPanel -- two buffers, the next panel's loads in flight under this panel's MFMAs, one barrier per panel --
// and BOTH operands' fragments are read transposed (RoundedPanel::frag_tr: ds_read_b64_tr_b16).
//
// The gather.  The x half of a panel row is the row of the edge's source id, clamped into [0, num_rows).  The ids of
// panel p + 2 are asked for right after the rows of panel p + 1, so no row load waits for its id inside the loop.
// The mask.  The keep word of a staged x float4 rides with it and is applied to the fp32 value -- kept: times scale --
// BEFORE the one rounding (RoundedPanel::edit), as in the forward's MASK 1 (edge_gemm16.hip).
//
// LDS image: row stride LD = 128 + TN elements when that is 32 x odd, else 32 more (288, 224, 160 elements for
// TN = 128, 64, 32: 576, 448, 320 bytes = 64 x {9, 7, 5}): a half's transposed read takes 4 consecutive rows x 64
// contiguous bytes, and 64 x odd bytes between rows put the four 16-bank runs at banks {0, 16, 32, 48} + const -- 64
// distinct banks, no conflict, for every TN (the section 2 rule of cdna_hip_programming.md; wgrad16.hip has the park).
//
// Rows past the end of a chunk are zeros in the image (they add nothing), never masked lanes; column sub-tiles of the
// 128 past M re-read a live sub-tile and are not stored: every lane runs every transposed read with EXEC all ones, and
// there is no `return` in the kernel.
//
// Determinism: a type with ONE chunk writes its tile straight to grad_w[t]; every other workgroup writes one fp32 partial
// tile to the workspace, and k_edge_wgrad16_reduce adds a type's partials in a fixed order -- eight lanes per output
// float4, each over chunks sub, sub + 8, ... ascending, then a fixed xor butterfly -- and writes zeros for a type without
// edges.  No atomics, no inline assembly; every store is a plain C++ assignment.
#include "half16.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

constexpr int kTM = 128;          // grad_msg columns (rows of grad_w) per workgroup tile
constexpr int kPE = 32;           // edges per panel: two MFMA k-steps
constexpr int kMinChunk = 512;    // edges
constexpr int kTargetGroups = 512;
constexpr int kSplit = 8;         // lanes per output float4 in the reduction
constexpr int kMaxTypes = 64;

struct ChunkOffsets {
  int32_t off[kMaxTypes + 1];     // prefix of edge chunks
  int32_t num_types;
};
struct EdgeWgrad16Table {
  const int64_t *src[kMaxTypes];
  int64_t edge_off[kMaxTypes + 1];   // prefix of edges: grad_msg (and mask) row of the type's edge 0
  ChunkOffsets chunks;
};

using GlobalIds = const __attribute__((address_space(1))) int64_t *;

inline int tile_n(int h) { return h % 128 == 0 ? 128 : (h % 64 == 0 ? 64 : 32); }
inline int64_t tiles_of(int m, int h) { return (int64_t)((m + kTM - 1) / kTM) * (h / tile_n(h)); }

inline int64_t chunk_edges_for(int64_t edges, int m, int h) {
  const int64_t want = (edges * tiles_of(m, h) + kTargetGroups - 1) / kTargetGroups;
  const int64_t c = (want + kPE - 1) / kPE * kPE;
  return c > kMinChunk ? c : kMinChunk;
}

template <int DT, int TN, bool MASK>
__global__ __launch_bounds__(256) void k_edge_wgrad16(EdgeWgrad16Table tab, const float *__restrict__ x, int64_t ld_x,
                                                      int64_t num_rows, int H, const float *__restrict__ g,
                                                      int64_t ld_g, int M, int64_t chunk_edges, int jtiles, int tiles,
                                                      const uint32_t *__restrict__ mask, float scale,
                                                      float *__restrict__ grad_w, float *__restrict__ partial) {
  using Hf = Half16<DT>;
  using vec = typename Hf::vec;
  constexpr int KT = kTM + TN;
  constexpr int LD = (KT / 32) % 2 == 1 ? KT : KT + 32;
  using Panel = RoundedPanel<DT, kPE, KT, LD>;
  constexpr int NJ = TN / 32, WJ = NJ >= 2 ? 2 : 1, WM = 4 / WJ, SM = 4 / WM, SJ = NJ / WJ;
  Panel panel;

  const int wave = threadIdx.x >> 6, li = frag_li();
  const int wm = wave / WJ, wn = wave % WJ;
  const int tile = (int)(blockIdx.x % tiles);
  const int chunk = (int)(blockIdx.x / tiles);          // < chunks.off[num_types]: the grid has no other workgroup
  int t = 0;
  for (int hi_t = tab.chunks.num_types; hi_t - t > 1;) {   // the last type whose first chunk is <= chunk: its owner
    const int mid = (t + hi_t) >> 1;
    if (tab.chunks.off[mid] <= chunk) t = mid; else hi_t = mid;
  }
  const int64_t row0 = tab.edge_off[t];                 // grad_msg / mask row of the type's edge 0
  const int64_t n_edges = tab.edge_off[t + 1] - row0;
  const int64_t e0 = (int64_t)(chunk - tab.chunks.off[t]) * chunk_edges;
  const int64_t e1 = e0 + chunk_edges < n_edges ? e0 + chunk_edges : n_edges;   // e1 > e0: a type has no empty chunk
  const int64_t num_panels = (e1 - e0 + kPE - 1) / kPE;
  const GlobalIds ids = (GlobalIds)tab.src[t];
  const int m0 = (tile / jtiles) * kTM, j0 = (tile % jtiles) * TN;
  const int mask_ld = H / 32;

  // Slot i of a thread is the same (row, columns) of every panel: columns < 128 are grad_msg's, the others x's.
  // nid[i]: the clamped source row of the NEXT panel to fetch, for the x slots.  An edge past the chunk's end asks for
  // the chunk's last edge (its row is never loaded: `live`).
  int nid[Panel::NV];
  uint32_t mw[MASK ? Panel::NV : 1];
  auto edge_of = [&](int64_t p, int r) {
    const int64_t e = e0 + p * kPE + r;
    return e < e1 ? e : e1 - 1;
  };
  auto fetch_ids = [&](int64_t p) {
#pragma unroll
    for (int i = 0; i < Panel::NV; ++i) {
      const int v = threadIdx.x + i * 256, r = v / Panel::RV, c = (v % Panel::RV) * 4;
      if (c >= kTM) {
        const int64_t id = ids[edge_of(p, r)];
        nid[i] = (int)(id < 0 ? 0 : (id < num_rows ? id : num_rows - 1));   // num_rows < 2^31 (the host checks)
      }
    }
  };
  auto fetch_mask = [&](int64_t p) {
#pragma unroll
    for (int i = 0; i < Panel::NV; ++i) {
      const int v = threadIdx.x + i * 256, r = v / Panel::RV, c = (v % Panel::RV) * 4;
      if (c >= kTM) mw[i] = mask[(row0 + edge_of(p, r)) * mask_ld + ((j0 + c - kTM) >> 5)];
    }
  };
  auto drop = [&](int i, int, int c, float4 &v) {
    if (c >= kTM) v = keep_scaled4(v, mw[i], (c - kTM) & 31, scale);   // j0 % 32 == 0
  };
  auto rows_of = [&](int64_t p) {        // panel p: [grad_msg columns m0 .. | x columns j0 ..] of edges e0 + 32 p ..
    return [&, p](int i, int r, int c) {
      const int gc = m0 + c < M ? m0 + c : m0 + c % 32;                   // a sub-tile past M: a live one, not stored
      return c < kTM ? g + (row0 + e0 + p * kPE + r) * ld_g + gc          // row < e1 wherever fetch dereferences
                     : x + (int64_t)nid[i] * ld_x + j0 + (c - kTM);
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

  fetch_ids(0);
  panel.fetch_slots(rows_of(0), live_of(0));
  if constexpr (MASK) fetch_mask(0);
  fetch_ids(1);
  if constexpr (MASK) panel.edit(drop);
  panel.start();
  for (int64_t p = 0; p < num_panels; ++p) {
    panel.fetch_slots(rows_of(p + 1), live_of(p + 1));  // past the last panel: live = 0, zeros, no load
    if constexpr (MASK) fetch_mask(p + 1);
    fetch_ids(p + 2);
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
        for (int b = 0; b < SJ; ++b) acc[a][b] = Hf::mfma(av[a], bv[b], acc[a][b]);
    }
    if constexpr (MASK) panel.edit(drop);
    panel.flip();
  }

  // the tile: register r of sub-tile (a, b) is grad_w[t][m0 + 32 (wm SM + a) + frag_row(r)][j0 + 32 (wn SJ + b) + li];
  // the type's only chunk writes it in place, every other chunk its partial
  const bool direct = tab.chunks.off[t + 1] - tab.chunks.off[t] == 1;
  float *pw = (direct ? grad_w + (int64_t)t * M * H : partial + (int64_t)chunk * M * H);
#pragma unroll
  for (int a = 0; a < SM; ++a) {
    const int ms = m0 + (wm * SM + a) * 32;
    if (ms < M) {                                       // wave-uniform; no transposed read follows
#pragma unroll
      for (int b = 0; b < SJ; ++b) {
        const int j = j0 + (wn * SJ + b) * 32 + li;
        for_frag_rows(ms, M, [&](int r, int64_t m) { pw[m * H + j] = acc[a][b][r]; });
      }
    }
  }
}

// grad_w[t][f] = sum over the type's chunks of partial[chunk][f], f a float4 of [M, H]: fixed order (file header).  A
// type with one chunk was written in place; a type without chunks gets zeros.
__global__ __launch_bounds__(256) void k_edge_wgrad16_reduce(ChunkOffsets chunks, const float *__restrict__ partial,
                                                             int64_t per_type4, float *__restrict__ grad_w) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t f = gid / kSplit;
  const int sub = (int)(gid % kSplit);
  if (f >= per_type4 * chunks.num_types) return;       // whole 8-lane groups leave together
  const int t = (int)(f / per_type4);
  const int64_t r = f % per_type4;
  const int c0 = chunks.off[t], c1 = chunks.off[t + 1];
  if (c1 - c0 == 1) return;                            // (the group's lanes share t)
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = c0 + sub; c < c1; c += kSplit) {
    const float4 v = *reinterpret_cast<const float4 *>(partial + ((int64_t)c * per_type4 + r) * 4);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
#pragma unroll
  for (int d = 1; d < kSplit; d <<= 1) {
    s.x += __shfl_xor(s.x, d); s.y += __shfl_xor(s.y, d);
    s.z += __shfl_xor(s.z, d); s.w += __shfl_xor(s.w, d);
  }
  if (sub == 0) *reinterpret_cast<float4 *>(grad_w + ((int64_t)t * per_type4 + r) * 4) = s;
}

bool shape_ok(int32_t state_dim, int32_t msg_dim, int32_t num_types) {
  return state_dim > 0 && state_dim % 32 == 0 && state_dim <= 1024 && msg_dim > 0 && msg_dim % 32 == 0 &&
         msg_dim <= 1024 && num_types >= 2 && num_types <= kMaxTypes;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_edge_weight_grad16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype) {
  return dtype_ok(dtype) && shape_ok(state_dim, msg_dim, num_types) ? 1 : 0;
}

extern "C" int64_t ptgnn_amd_edge_wgrad16_chunk_edges(int64_t num_edges, int32_t num_types, int32_t msg_dim,
                                                      int32_t state_dim) {
  if (num_edges < 0 || !shape_ok(state_dim, msg_dim, num_types)) return 0;
  return chunk_edges_for(num_edges, msg_dim, state_dim);
}

extern "C" size_t ptgnn_amd_edge_wgrad16_workspace_bytes(int64_t num_edges, int32_t num_types, int32_t msg_dim,
                                                         int32_t state_dim) {
  if (num_edges <= 0 || !shape_ok(state_dim, msg_dim, num_types)) return 0;
  const int64_t chunks = num_edges / chunk_edges_for(num_edges, msg_dim, state_dim) + num_types;   // >= sum_t ceil(E_t / it)
  return (size_t)chunks * (size_t)msg_dim * (size_t)state_dim * sizeof(float);
}

extern "C" int ptgnn_amd_edge_weight_grad16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                            const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                            const float *grad_msg, int64_t ld_grad_msg, int32_t num_types,
                                            int32_t msg_dim, int dtype, float dropout_p, const uint32_t *mask_bits,
                                            float *grad_w, void *workspace, size_t workspace_bytes, void *stream_) {
  PTGNN_REQUIRE(num_types > 0 && state_dim > 0 && msg_dim > 0, PTGNN_AMD_EINVAL, "edge_weight_grad16: bad sizes");
  PTGNN_REQUIRE(dtype_ok(dtype), PTGNN_AMD_EINVAL, "edge_weight_grad16: dtype %d is neither PTGNN_AMD_HALF_BF16 nor _F16",
                dtype);
  PTGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, PTGNN_AMD_EINVAL, "edge_weight_grad16: bad dropout p");
  PTGNN_REQUIRE(shape_ok(state_dim, msg_dim, num_types), PTGNN_AMD_EUNSUPPORTED,
                "edge_weight_grad16: state_dim=%d msg_dim=%d num_types=%d: needs both widths %% 32 == 0 and <= 1024, "
                "2 <= num_types <= %d", state_dim, msg_dim, num_types, kMaxTypes);
  PTGNN_REQUIRE(edges_per_type && grad_w, PTGNN_AMD_EINVAL, "edge_weight_grad16: null pointer");
  PTGNN_REQUIRE(aligned16(grad_w), PTGNN_AMD_EUNSUPPORTED, "edge_weight_grad16: grad_w must be 16-byte aligned");
  int64_t E = 0;
  for (int t = 0; t < num_types; ++t) {
    PTGNN_REQUIRE(edges_per_type[t] >= 0, PTGNN_AMD_EINVAL, "edge_weight_grad16: negative edge count of type %d", t);
    E += edges_per_type[t];
  }
  hipStream_t st = (hipStream_t)stream_;
  const size_t out_bytes = (size_t)num_types * msg_dim * state_dim * sizeof(float);
  if (E == 0) {   // zeros, no launch
    PTGNN_HIP(hipMemsetAsync(grad_w, 0, out_bytes, st));
    return PTGNN_AMD_OK;
  }
  PTGNN_REQUIRE(x && src_per_type && grad_msg, PTGNN_AMD_EINVAL, "edge_weight_grad16: null pointer");
  PTGNN_REQUIRE(num_rows > 0 && ld_x >= state_dim && ld_grad_msg >= msg_dim, PTGNN_AMD_EINVAL,
                "edge_weight_grad16: num_rows must be positive, ld_x >= state_dim and ld_grad_msg >= msg_dim");
  PTGNN_REQUIRE(num_rows < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "edge_weight_grad16: too many rows of x");
  PTGNN_REQUIRE(rows16(x, ld_x) && rows16(grad_msg, ld_grad_msg), PTGNN_AMD_EUNSUPPORTED,
                "edge_weight_grad16: x and grad_msg must be 16-byte aligned with ld %% 4 == 0 (ld_x=%lld, "
                "ld_grad_msg=%lld)", (long long)ld_x, (long long)ld_grad_msg);
  const bool masked = mask_bits != nullptr && dropout_p > 0.f;
  PTGNN_REQUIRE(!masked || aligned4(mask_bits), PTGNN_AMD_EUNSUPPORTED,
                "edge_weight_grad16: mask_bits must be 4-byte aligned");
  const int64_t ch = chunk_edges_for(E, msg_dim, state_dim);
  EdgeWgrad16Table tab;
  tab.chunks.num_types = num_types;
  tab.edge_off[0] = 0;
  tab.chunks.off[0] = 0;
  for (int t = 0; t < num_types; ++t) {
    const int64_t n = edges_per_type[t];
    PTGNN_REQUIRE(n == 0 || src_per_type[t], PTGNN_AMD_EINVAL, "edge_weight_grad16: null source ids of type %d", t);
    tab.src[t] = n ? src_per_type[t] : nullptr;
    tab.edge_off[t + 1] = tab.edge_off[t] + n;
    const int64_t chunks = tab.chunks.off[t] + (n + ch - 1) / ch;
    PTGNN_REQUIRE(chunks < ((int64_t)1 << 30), PTGNN_AMD_EUNSUPPORTED, "edge_weight_grad16: too many chunks");
    tab.chunks.off[t + 1] = (int32_t)chunks;
  }
  for (int t = num_types; t < kMaxTypes; ++t) {
    tab.src[t] = nullptr;
    tab.edge_off[t + 1] = tab.edge_off[num_types];
    tab.chunks.off[t + 1] = tab.chunks.off[num_types];
  }
  const int64_t chunks = tab.chunks.off[num_types];     // <= E / ch + num_types: what the workspace was sized for
  const int tn = tile_n(state_dim), jtiles = state_dim / tn;
  const int64_t tiles = tiles_of(msg_dim, state_dim), blocks = tiles * chunks;
  PTGNN_REQUIRE(blocks < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "edge_weight_grad16: too many tiles");
  const size_t need = ptgnn_amd_edge_wgrad16_workspace_bytes(E, num_types, msg_dim, state_dim);
  PTGNN_REQUIRE(workspace_bytes >= need && workspace && aligned16(workspace), PTGNN_AMD_EINVAL,
                "edge_weight_grad16: workspace too small or unaligned (%zu bytes, needs %zu)", workspace_bytes, need);
  float *partial = static_cast<float *>(workspace);
  const float scale = masked ? 1.0f / (1.0f - dropout_p) : 1.0f;
  with_dtype(dtype, [&](auto dt) {
    with_case<128, 64, 32>(tn, [&](auto tnc) {
      constexpr int DT = decltype(dt)::value, TN = decltype(tnc)::value;
      if (masked)
        k_edge_wgrad16<DT, TN, true><<<(unsigned)blocks, 256, 0, st>>>(tab, x, ld_x, num_rows, state_dim, grad_msg,
                                                                      ld_grad_msg, msg_dim, ch, jtiles, (int)tiles,
                                                                      mask_bits, scale, grad_w, partial);
      else
        k_edge_wgrad16<DT, TN, false><<<(unsigned)blocks, 256, 0, st>>>(tab, x, ld_x, num_rows, state_dim, grad_msg,
                                                                       ld_grad_msg, msg_dim, ch, jtiles, (int)tiles,
                                                                       nullptr, scale, grad_w, partial);
    });
  });
  PTGNN_LAUNCH_CHECK();
  const int64_t per_type4 = (int64_t)msg_dim * state_dim / 4;
  k_edge_wgrad16_reduce<<<(unsigned)((per_type4 * num_types * kSplit + 255) / 256), 256, 0, st>>>(tab.chunks, partial,
                                                                                                 per_type4, grad_w);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_EDGE_WGRAD16);
  return PTGNN_AMD_OK;
}
