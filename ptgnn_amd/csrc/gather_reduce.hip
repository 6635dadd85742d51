// Fused gather -> (+dst term) -> segment reduce -> (GELU / LayerNorm) over a dst-sorted CSR.
// Contract + reference lines: include/ptgnn_amd.h (ptgnn_amd_gather_reduce_f32).
// The row walk, the hub / long-row launches and their plumbing live in gather_reduce_core.h.
#include "gather_reduce_core.h"

namespace ptgnn_amd {
namespace {
constexpr int kSidePool = 64;
std::mutex g_side_mu;
SideStream g_side[kSidePool];
int g_side_used = 0;

bool side_streams_enabled() {
  static const bool enabled = [] {
    const char *e = getenv("PTGNN_AMD_HUB_STREAM");
    return !(e && e[0] == '0');
  }();
  return enabled;
}
}  // namespace

// the caller stream's set, created if `may_create` (not capturing) and there is room; else nullptr
SideStream *side_stream(hipStream_t caller, bool may_create) {
  if (!side_streams_enabled()) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_side_mu);
  for (int i = 0; i < g_side_used; ++i)
    if (g_side[i].dev == dev && g_side[i].owner == caller) return &g_side[i];
  if (!may_create || g_side_used == kSidePool) return nullptr;
  SideStream &s = g_side[g_side_used];
  if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&s.stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s.join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s.join2, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;                // a half-created set is never published (its handles leak once, on a failing device)
  }
  s.dev = dev;
  s.owner = caller;
  ++g_side_used;
  return &s;
}

namespace {

// ------------------------------------------------------------------------------------------------
// aggregation + node update of the MLP-MP layer in ONE kernel (hidden 64: the README's default architecture, BASELINE
// config 4):  out[v] = act(W . LayerNorm(GELU(aggregate[v])) + b)       (mlpmessagepassing.py:107-117, :56-66)
// ------------------------------------------------------------------------------------------------
// At M = 64 the dense update is a [N, 64] x [64, H'] GEMM with 16 KB of weights: as a launch of its own it reads and
// writes [N, 64] once more and costs 17-21 us per layer against an ~11 us copy floor (profiles/r04: `linear` 0.33 of the MFMA
// peak, i.e. it is a memory pass).  Here a workgroup of 8 waves aggregates 32 destination rows exactly as k_gather_reduce
// does (a row per 16-lane group, CSR order, the same prefetched groups of 8 slots, GELU + LayerNorm in registers), parks
// the 32 normalised rows in LDS, and its eight waves multiply the tile with the weight matrix -- copied into LDS at the
// start of the workgroup, behind the first gather round trip -- on the matrix cores in the library's one K order
// (`kcol`), add the bias, apply the activation and store their 16 x 16 tiles.  Same bits as
// ptgnn_amd_gather_reduce_f32 followed by ptgnn_amd_linear_f32.  The aggregate never exists in memory.
// Every row folds serially in slot order here, whatever its length (no hub / long-row launches): the host takes this
// kernel for minibatch-sized plans only, where a row beyond a few hundred in-edges is an oddity, not a workload -- and
// stops taking it for a while when a plan reports hub rows (ptgnn_amd.ops.gather_update_supported reads the plan's hub
// count back asynchronously).  A workgroup-cooperative fold of such rows inside this kernel was built and dropped: its
// second fold loop raised the allocation from 62-72 to 76-96 VGPRs, i.e. from four resident workgroups per CU to two,
// on the path that has no hub rows.
struct UpdateArgs {
  const float *w;      // [out_dim, M] row-major (nn.Linear layout)
  const float *bias;   // nullable
  int32_t out_dim;     // 32 | 64 | 96 | 128
  int32_t act;
  float *out;          // [num_nodes, out_dim]
  int64_t ld_out;
};

constexpr int kUpdM = 64;             // message width of the fused form
constexpr int kUpdLd = kUpdM + 4;     // LDS row stride: 16-byte aligned rows, conflict-free ds_read_b128 of the MFMA fragments

using f32x4v = __attribute__((ext_vector_type(4))) float;

// The tile product runs on v_mfma_f32_16x16x4_f32, one 16 x 16 output tile per wave: all eight waves of the workgroup
// multiply (16 MFMAs each).  The four k of an instruction are (kcol(s), kcol(s) + 4, kcol(s + 1), kcol(s + 1) + 4): the
// products of a row meet the accumulator in the SAME order as in two 32x32x2 steps of the GEMM kernels, hence the same bits
// (asserted on the GPU against gather_reduce + linear, tests/test_gpu_gather_update.py).  Measured alternatives (cfg4, per
// layer; profiles/r05_notes.md 2): unfused 50.1 us; this form 42.2 us; the tile on 32x32x2 (two of the eight waves multiply,
// rows leave through LDS) 45.8 us; wave-local products on v_mfma_f32_4x4x1 -- no barrier behind the gather -- 53.0 us, and
// the same with persistent workgroups (weights loaded once) 56.3 us: a chain of 64 dependent 4x4x1 MFMAs per row quad costs
// more than the barrier it avoids.
template <int REDUCE>
__global__ __launch_bounds__(512) void k_gather_update(Args a, UpdateArgs u) {
  extern __shared__ __attribute__((aligned(16))) float upd_smem[];
  constexpr int LPR = 16, ROWS = 32;
  float *const Ws = upd_smem;                                   // [out_dim][kUpdLd]
  float *const As = Ws + u.out_dim * kUpdLd;                    // [32][kUpdLd]  normalised rows
  const int64_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= a.num_tiles) return;                               // workgroup-uniform
  // the weights: issued first, they travel behind the rowptr / col / row round trips of the gather below
  // (held in registers until the gather is done: a load -> ds_write pair up front would wait for the load right here)
  const int wq = u.out_dim * (kUpdM / 4);                        // float4 pieces of W: 512 .. 2048
  float4 wv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = (int)threadIdx.x + j * 512;
    const int ic = i < wq ? i : wq - 1;
    wv[j] = *reinterpret_cast<const float4 *>(u.w + (int64_t)(ic >> 4) * kUpdM + (ic & 15) * 4);
  }
  const int grp = threadIdx.x / LPR, g = threadIdx.x % LPR;
  const int64_t row0 = a.row_begin + tile * ROWS;
  const int64_t row = row0 + grp;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  {
    RowOp<4, LPR, 1, REDUCE, false, false, false> op(a, g, 0);
    if (row < a.num_nodes) {
      const int beg = a.rowptr[row], end = a.rowptr[row + 1];
      op.template reduce_pf<8>(row, beg, end, 1);
      op.finish(end - beg);
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) op.acc[0][v] = 0.f;            // rows past the end: computed, never stored
    }
    *reinterpret_cast<float4 *>(As + grp * kUpdLd + g * 4) = make_float4(op.acc[0][0], op.acc[0][1], op.acc[0][2], op.acc[0][3]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = (int)threadIdx.x + j * 512;
    if (i < wq) *reinterpret_cast<float4 *>(Ws + (i >> 4) * kUpdLd + (i & 15) * 4) = wv[j];
  }
  __syncthreads();
  auto activate = [&](float v) {
    return u.act == PTGNN_AMD_ACT_TANH ? act_apply<PTGNN_AMD_ACT_TANH>(v)
                                       : (u.act == PTGNN_AMD_ACT_RELU ? act_apply<PTGNN_AMD_ACT_RELU>(v) : v);
  };
  {
    // tile t = (row half, 16-column block): waves stride over the 2 * out_dim / 16 tiles (8 at out_dim 64: one each)
    const int r16 = lane & 15, kq = lane >> 4;
    const int koff = (kq & 1) * 4 + (kq >> 1);                   // this lane's k inside an instruction: base + {0, 4, 1, 5}[kq]
    const int ntiles = u.out_dim >> 3;                           // 2 * (out_dim / 16)
    for (int t = wave; t < ntiles; t += 8) {
      const int rh = t & 1, cb = t >> 1;
      const float *al = As + (rh * 16 + r16) * kUpdLd + koff;
      const float *bl = Ws + (cb * 16 + r16) * kUpdLd + koff;
      f32x4v c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ch = 0; ch < kUpdM / 32; ++ch)
#pragma unroll
        for (int jp = 0; jp < 8; ++jp) {                          // MFMA steps 2 jp, 2 jp + 1 of the 32x32x2 kernels
          const int base = ch * 32 + (jp >> 1) * 8 + (jp & 1) * 2;
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(al[base], bl[base], c, 0, 0, 0);
        }
      const int colx = cb * 16 + r16;
      const float b = u.bias ? u.bias[colx] : 0.f;
      // C fragment: column r16, rows 4 kq + {0..3} of the 16-row half
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t orow = row0 + rh * 16 + 4 * kq + i;
        const float v = u.bias ? c[i] + b : c[i];
        if (orow < a.num_nodes) u.out[orow * u.ld_out + colx] = activate(v);
      }
    }
  }
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int64_t ptgnn_amd_hub_ticket_count(int64_t num_edges, int32_t msg_dim) {
  if (num_edges <= 0 || msg_dim <= 0) return 0;
  // one counter per (chunk, column block); column blocks only exist beyond 512 columns
  const int64_t col_blocks = msg_dim <= 512 ? 1 : (msg_dim + 255) / 256;
  return (num_edges + kHubChunk - 1) / kHubChunk * col_blocks;
}

extern "C" size_t ptgnn_amd_hub_workspace_bytes(int64_t num_edges, int32_t msg_dim, int with_arg) {
  if (num_edges <= 0 || msg_dim <= 0) return 0;
  const size_t chunks = (size_t)((num_edges + kHubChunk - 1) / kHubChunk);
  return 2 * chunks * (size_t)msg_dim * 4 * (with_arg ? 2 : 1) + 256;
}

extern "C" int ptgnn_amd_gather_reduce_f32(const float *ysrc, int64_t ld_y, const float *ydst,
                                           int64_t ld_yd, const int32_t *rowptr, const int32_t *col,
                                           int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                           int reduce, int epilogue, const float *ln_gamma,
                                           const float *ln_beta, float ln_eps, float *out,
                                           int64_t ld_out, int32_t *argout, int64_t num_edges,
                                           int32_t hub_threshold, const int32_t *hub_entries,
                                           const int32_t *hub_count, void *hub_ws,
                                           size_t hub_ws_bytes, int32_t *hub_tickets, void *stream_) {
  return ptgnn_amd_gather_reduce_rows_f32(ysrc, ld_y, ydst, ld_yd, rowptr, col, type_bits, num_nodes, msg_dim, reduce,
                                          epilogue, ln_gamma, ln_beta, ln_eps, out, ld_out, argout, num_edges,
                                          hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes, hub_tickets, 0,
                                          num_nodes, stream_);
}

extern "C" int ptgnn_amd_gather_reduce_rows_f32(const float *ysrc, int64_t ld_y, const float *ydst,
                                                int64_t ld_yd, const int32_t *rowptr, const int32_t *col,
                                                int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                                int reduce, int epilogue, const float *ln_gamma,
                                                const float *ln_beta, float ln_eps, float *out,
                                                int64_t ld_out, int32_t *argout, int64_t num_edges,
                                                int32_t hub_threshold, const int32_t *hub_entries,
                                                const int32_t *hub_count, void *hub_ws,
                                                size_t hub_ws_bytes, int32_t *hub_tickets, int64_t row_begin,
                                                int64_t row_end, void *stream_) {
  return ptgnn_amd_gather_reduce_hdr_f32(ysrc, ld_y, ydst, ld_yd, rowptr, col, type_bits, num_nodes, msg_dim, reduce,
                                         epilogue, ln_gamma, ln_beta, ln_eps, out, ld_out, argout, num_edges,
                                         hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes, hub_tickets,
                                         row_begin, row_end, nullptr, stream_);
}

extern "C" int ptgnn_amd_gather_reduce_hdr_f32(const float *ysrc, int64_t ld_y, const float *ydst,
                                               int64_t ld_yd, const int32_t *rowptr, const int32_t *col,
                                               int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                               int reduce, int epilogue, const float *ln_gamma,
                                               const float *ln_beta, float ln_eps, float *out,
                                               int64_t ld_out, int32_t *argout, int64_t num_edges,
                                               int32_t hub_threshold, const int32_t *hub_entries,
                                               const int32_t *hub_count, void *hub_ws,
                                               size_t hub_ws_bytes, int32_t *hub_tickets, int64_t row_begin,
                                               int64_t row_end, const int32_t *row_hdr, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PTGNN_REQUIRE(num_nodes >= 0 && msg_dim > 0 && num_edges >= 0, PTGNN_AMD_EINVAL, "gather_reduce: bad sizes");
  PTGNN_REQUIRE(((uintptr_t)row_hdr & 31) == 0, PTGNN_AMD_EINVAL, "gather_reduce: row_hdr must be 32-byte aligned");
  PTGNN_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= num_nodes, PTGNN_AMD_EINVAL,
                "gather_reduce: row range [%lld, %lld) outside [0, %lld]", (long long)row_begin, (long long)row_end,
                (long long)num_nodes);
  if (row_begin == row_end) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "gather_reduce: unknown reduce %d", reduce);
  PTGNN_REQUIRE(epilogue >= 0 && epilogue <= 3, PTGNN_AMD_EINVAL, "gather_reduce: bad epilogue");
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "gather_reduce: bad type_bits");
  if (num_nodes == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && out && ld_out >= msg_dim, PTGNN_AMD_EINVAL, "gather_reduce: null/ld");
  // a plan without edges (every edge type of the minibatch empty) reads no message row: its table may be a null pointer
  PTGNN_REQUIRE(col && (ysrc || num_edges == 0), PTGNN_AMD_EINVAL, "gather_reduce: null ysrc/col");
  PTGNN_REQUIRE(!(epilogue & PTGNN_AMD_EPI_LAYERNORM) || (ln_gamma && ln_beta), PTGNN_AMD_EINVAL,
                "gather_reduce: LayerNorm epilogue needs gamma/beta");
  PTGNN_REQUIRE(argout == nullptr || reduce >= PTGNN_AMD_MAX, PTGNN_AMD_EINVAL,
                "gather_reduce: argout only with max/min");

  Args a{};
  a.ysrc = ysrc; a.ydst = ydst; a.ld_y = ld_y; a.ld_yd = ydst ? ld_yd : ld_y;
  a.rowptr = rowptr; a.col = col; a.type_bits = type_bits; a.num_nodes = row_end; a.row_begin = row_begin; a.msg_dim = msg_dim;
  a.ln_gamma = ln_gamma; a.ln_beta = ln_beta; a.ln_eps = ln_eps; a.out = out; a.ld_out = ld_out;
  a.argout = argout; a.epi = epilogue;
  a.hdr = row_hdr;   // read by the walks in groups of 8 only (gather_reduce_core.h); every other variant ignores it
  const int rc = setup_hub(a, num_edges, hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes,
                           hub_tickets, argout != nullptr);
  if (rc != PTGNN_AMD_OK) return rc;
  const bool vec4 = (msg_dim % 4 == 0) && (ld_y % 4 == 0) && (!ydst || ld_yd % 4 == 0) && (ld_out % 4 == 0) &&
                    aligned16(ysrc) && aligned16(out) && (!ydst || aligned16(ydst)) &&
                    (!argout || aligned16(argout));
  const bool row_epi = (epilogue & PTGNN_AMD_EPI_LAYERNORM) != 0;
  const int rc2 = dispatch_geometry(vec4, msg_dim, row_epi, [&](auto V, auto L, auto C, int col_blocks) {
    return launch1<decltype(V)::value, decltype(L)::value, decltype(C)::value>(a, reduce, col_blocks, stream);
  });
  if (rc2 == PTGNN_AMD_OK) count_launch(PTGNN_AMD_KERNEL_GATHER_REDUCE);
  return rc2;
}

extern "C" int ptgnn_amd_gather_update_supported(int32_t msg_dim, int32_t out_dim) {
  return msg_dim == kUpdM && out_dim >= 32 && out_dim <= 128 && out_dim % 32 == 0 ? 1 : 0;
}

extern "C" int ptgnn_amd_gather_update_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr, const int32_t *col,
                                           int32_t type_bits, int64_t num_nodes, int32_t msg_dim, int reduce,
                                           int epilogue, const float *ln_gamma, const float *ln_beta, float ln_eps,
                                           const float *w, const float *bias, int32_t out_dim, int act, float *out,
                                           int64_t ld_out, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0, PTGNN_AMD_EINVAL, "gather_update: bad sizes");
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL, "gather_update: unknown reduce %d", reduce);
  PTGNN_REQUIRE(epilogue >= 0 && epilogue <= 3, PTGNN_AMD_EINVAL, "gather_update: bad epilogue");
  PTGNN_REQUIRE(act >= 0 && act <= PTGNN_AMD_ACT_RELU, PTGNN_AMD_EINVAL, "gather_update: bad act");
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "gather_update: bad type_bits");
  PTGNN_REQUIRE(ptgnn_amd_gather_update_supported(msg_dim, out_dim), PTGNN_AMD_EUNSUPPORTED,
                "gather_update: msg_dim=%d out_dim=%d is not a shape of the fused kernel (msg_dim 64, out_dim 32..128 in "
                "steps of 32)", msg_dim, out_dim);
  if (num_nodes == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(msg && rowptr && col && w && out && ld_out >= out_dim, PTGNN_AMD_EINVAL, "gather_update: null/ld");
  PTGNN_REQUIRE(!(epilogue & PTGNN_AMD_EPI_LAYERNORM) || (ln_gamma && ln_beta), PTGNN_AMD_EINVAL,
                "gather_update: LayerNorm epilogue needs gamma/beta");
  PTGNN_REQUIRE(ld_msg % 4 == 0 && ld_out % 4 == 0 && aligned16(msg) && aligned16(out) && aligned16(w), PTGNN_AMD_EUNSUPPORTED,
                "gather_update: rows must be 16-byte aligned");
  Args a{};
  a.ysrc = msg; a.ydst = nullptr; a.ld_y = ld_msg; a.ld_yd = ld_msg;
  a.rowptr = rowptr; a.col = col; a.type_bits = type_bits; a.num_nodes = num_nodes; a.row_begin = 0; a.msg_dim = msg_dim;
  a.ln_gamma = ln_gamma; a.ln_beta = ln_beta; a.ln_eps = ln_eps; a.out = nullptr; a.ld_out = 0; a.argout = nullptr;
  a.epi = epilogue;
  a.num_tiles = (num_nodes + 31) / 32;
  UpdateArgs u;
  u.w = w; u.bias = bias; u.out_dim = out_dim; u.act = act; u.out = out; u.ld_out = ld_out;
  // A/B + bit-identity test knob: PTGNN_AMD_GATHER_UPDATE_MFMA=32 takes the 32x32x2 form of the tile product
  const size_t lds = ((size_t)out_dim * kUpdLd + 32 * kUpdLd) * sizeof(float);
  const unsigned grid = (unsigned)xcd_padded_blocks(a.num_tiles);
  hipStream_t st = (hipStream_t)stream_;
  switch (reduce) {
    case PTGNN_AMD_SUM: k_gather_update<PTGNN_AMD_SUM><<<grid, 512, lds, st>>>(a, u); break;
    case PTGNN_AMD_MEAN: k_gather_update<PTGNN_AMD_MEAN><<<grid, 512, lds, st>>>(a, u); break;
    case PTGNN_AMD_MAX: k_gather_update<PTGNN_AMD_MAX><<<grid, 512, lds, st>>>(a, u); break;
    default: k_gather_update<PTGNN_AMD_MIN><<<grid, 512, lds, st>>>(a, u); break;
  }
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_GATHER_UPDATE);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_gather_reduce_masked_f32(const float *grad, int64_t ld_grad,
                                                  const int32_t *arg, const int32_t *rowptr,
                                                  const int32_t *col, const int32_t *slot_of,
                                                  int64_t num_rows, int32_t msg_dim, float *out,
                                                  int64_t ld_out, int64_t num_edges,
                                                  int32_t hub_threshold, const int32_t *hub_entries,
                                                  const int32_t *hub_count, void *hub_ws,
                                                  size_t hub_ws_bytes, int32_t *hub_tickets,
                                                  void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  PTGNN_REQUIRE(num_rows >= 0 && msg_dim > 0 && num_edges >= 0, PTGNN_AMD_EINVAL,
                "gather_reduce_masked: bad sizes");
  if (num_rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(grad && arg && rowptr && col && slot_of && out && ld_out >= msg_dim && ld_grad >= msg_dim,
                PTGNN_AMD_EINVAL, "gather_reduce_masked: null/ld");
  Args a{};
  a.ysrc = grad; a.ld_y = ld_grad; a.ld_yd = ld_grad; a.rowptr = rowptr; a.col = col;
  a.num_nodes = num_rows; a.msg_dim = msg_dim; a.out = out; a.ld_out = ld_out;
  a.mask_arg = arg; a.mask_slot = slot_of;
  const int rc = setup_hub(a, num_edges, hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes,
                           hub_tickets, false);
  if (rc != PTGNN_AMD_OK) return rc;
  const bool vec4 = (msg_dim % 4 == 0) && (ld_grad % 4 == 0) && (ld_out % 4 == 0) && aligned16(grad) &&
                    aligned16(out) && aligned16(arg);
  return dispatch_geometry(vec4, msg_dim, false, [&](auto V, auto L, auto C, int col_blocks) {
    return launch_all<decltype(V)::value, decltype(L)::value, decltype(C)::value, PTGNN_AMD_SUM, false, false,
                      true>(a, col_blocks, stream);
  });
}

// ---------------------------------------------------------------------------------------------
// row headers of a plan: hdr[r, k] = entries[min(rowptr[r] + k, rowptr[r + 1] - 1)], zeros for an empty row
// ---------------------------------------------------------------------------------------------
namespace ptgnn_amd {
namespace {
// one thread per header entry: the eight threads of a row read the same rowptr pair (one 8-byte request after
// coalescing) and write one 32-byte record; ~4 MB of traffic for the 116 k rows of BASELINE config 3
__global__ __launch_bounds__(256) void k_row_headers(const int32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ entries, int64_t num_rows,
                                                     int32_t *__restrict__ hdr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = i >> 3;
  if (r >= num_rows) return;
  const int k = (int)(i & 7);
  const int beg = rowptr[r], end = rowptr[r + 1];
  int32_t v = 0;
  if (end > beg) v = entries[beg + k < end ? beg + k : end - 1];
  hdr[i] = v;
}
}  // namespace
}  // namespace ptgnn_amd

extern "C" int ptgnn_amd_row_headers(const int32_t *rowptr, const int32_t *entries, int64_t num_rows, int32_t *hdr,
                                     void *stream_) {
  PTGNN_REQUIRE(num_rows >= 0 && num_rows < ((int64_t)1 << 31), PTGNN_AMD_EINVAL, "row_headers: bad sizes");
  if (num_rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && entries && hdr, PTGNN_AMD_EINVAL, "row_headers: null pointer");
  PTGNN_REQUIRE(((uintptr_t)hdr & 31) == 0, PTGNN_AMD_EINVAL, "row_headers: hdr must be 32-byte aligned");
  const int64_t blocks = (num_rows * 8 + 255) / 256;
  k_row_headers<<<(unsigned)blocks, 256, 0, (hipStream_t)stream_>>>(rowptr, entries, num_rows, hdr);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

// ---------------------------------------------------------------------------------------------
// plain row gather (general per-edge path + task-head indexing)
// ---------------------------------------------------------------------------------------------
namespace ptgnn_amd {
namespace {
__global__ __launch_bounds__(256) void k_gather_rows(const float *__restrict__ x, int64_t ld_x,
                                                     const int64_t *__restrict__ idx,
                                                     int64_t n_idx, int dim,
                                                     float *__restrict__ out, int64_t ld_out,
                                                     int vec4) {
  // one wave per output row, lanes stride the row
  const int lane = threadIdx.x & 63;
  const int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = w; r < n_idx; r += nw) {
    const float *src = x + idx[r] * ld_x;
    float *dst = out + r * ld_out;
    if (vec4) {
      for (int c = lane * 4; c < dim; c += 256)
        *reinterpret_cast<float4 *>(dst + c) = *reinterpret_cast<const float4 *>(src + c);
    } else {
      for (int c = lane; c < dim; c += 64) dst[c] = src[c];
    }
  }
}
}  // namespace
}  // namespace ptgnn_amd

extern "C" int ptgnn_amd_gather_rows_f32(const float *x, int64_t ld_x, const int64_t *idx,
                                         int64_t n_idx, int32_t dim, float *out, int64_t ld_out,
                                         void *stream_) {
  PTGNN_REQUIRE(n_idx >= 0 && dim > 0, PTGNN_AMD_EINVAL, "gather_rows: bad sizes");
  if (n_idx == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(x && idx && out, PTGNN_AMD_EINVAL, "gather_rows: null pointer");
  const int vec4 = (dim % 4 == 0) && (ld_x % 4 == 0) && (ld_out % 4 == 0) && aligned16(x) && aligned16(out);
  int64_t blocks = (n_idx + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  k_gather_rows<<<(unsigned)blocks, 256, 0, (hipStream_t)stream_>>>(x, ld_x, idx, n_idx, dim, out,
                                                                    ld_out, vec4);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

// ---------------------------------------------------------------------------------------------
// Backward of the segment reduce: spread the output-row gradients back onto the message rows.
//   d_msg[perm[s], :] = grad[row(s), :]                      sum (mean: the caller pre-divides grad)
//   d_msg[perm[s], c] = arg[row(s), c] == s ? grad[row(s), c] : 0     max / min (torch_scatter arg_out)
// One CSR slot per group of dim/4 lanes; the slot -> row map is the plan's expanded rowptr.  Reads of
// `grad` are row-sequential (slots of a row are adjacent), every message row is written exactly once
// as a whole row, so there is nothing to zero-fill and nothing to accumulate.
// ---------------------------------------------------------------------------------------------
namespace ptgnn_amd {
namespace {
template <bool VEC4>
__global__ __launch_bounds__(256) void k_segment_spread(const float *__restrict__ grad, int64_t ld_grad,
                                                        const int32_t *__restrict__ arg,
                                                        const int32_t *__restrict__ slot_row,
                                                        const int32_t *__restrict__ perm,
                                                        int64_t num_slots, int dim,
                                                        float *__restrict__ out, int64_t ld_out) {
  const int q = VEC4 ? dim / 4 : dim;                 // work items per slot
  const int64_t total = num_slots * q;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t s = i / q;
    const int c = (int)(i - s * q) * (VEC4 ? 4 : 1);
    const int64_t row = slot_row[s];
    const int64_t e = perm[s];
    if constexpr (VEC4) {
      float4 g = *reinterpret_cast<const float4 *>(grad + row * ld_grad + c);
      if (arg) {
        const int4 a = *reinterpret_cast<const int4 *>(arg + row * dim + c);
        const int32_t si = (int32_t)s;
        g.x = a.x == si ? g.x : 0.f; g.y = a.y == si ? g.y : 0.f;
        g.z = a.z == si ? g.z : 0.f; g.w = a.w == si ? g.w : 0.f;
      }
      *reinterpret_cast<float4 *>(out + e * ld_out + c) = g;
    } else {
      float g = grad[row * ld_grad + c];
      if (arg && arg[row * dim + c] != (int32_t)s) g = 0.f;
      out[e * ld_out + c] = g;
    }
  }
}

// The widths the layers use (dim = 4 LPR, LPR in {16, 32, 64}; float4 rows): one slot per group of LPR lanes, SPG slots
// per group and pass with all their loads requested up front.  The generic kernel above spends a 64-bit division per
// item and has one dependent chain (slot -> row index -> gradient row -> store) per thread in flight: 0.46-0.50 of HBM
// on the training step's [625 k, 128] / [625 k, 64] spreads (profiles/r03_notes.md).
template <int LPR, int SPG, bool HAS_ARG>
__global__ __launch_bounds__(256) void k_segment_spread_rows(const float *__restrict__ grad, int64_t ld_grad,
                                                             const int32_t *__restrict__ arg,
                                                             const int32_t *__restrict__ slot_row,
                                                             const int32_t *__restrict__ perm, int64_t num_slots,
                                                             float *__restrict__ out, int64_t ld_out) {
  constexpr int G = 256 / LPR, DIM = 4 * LPR;
  const int g = threadIdx.x % LPR, c = 4 * g;
  const int64_t s0 = ((int64_t)blockIdx.x * G + threadIdx.x / LPR) * SPG;
  if (s0 >= num_slots) return;
  int64_t row[SPG], e[SPG];
#pragma unroll
  for (int k = 0; k < SPG; ++k) {
    const int64_t s = s0 + k < num_slots ? s0 + k : num_slots - 1;
    row[k] = slot_row[s];
    e[k] = perm[s];
  }
  float4 v[SPG];
  int4 a[SPG];
#pragma unroll
  for (int k = 0; k < SPG; ++k) {
    v[k] = *reinterpret_cast<const float4 *>(grad + row[k] * ld_grad + c);
    if constexpr (HAS_ARG) a[k] = *reinterpret_cast<const int4 *>(arg + row[k] * DIM + c);
  }
#pragma unroll
  for (int k = 0; k < SPG; ++k) {
    if (s0 + k >= num_slots) break;                   // uniform inside the lane group
    float4 o = v[k];
    if constexpr (HAS_ARG) {
      const int32_t si = (int32_t)(s0 + k);
      o.x = a[k].x == si ? o.x : 0.f; o.y = a[k].y == si ? o.y : 0.f;
      o.z = a[k].z == si ? o.z : 0.f; o.w = a[k].w == si ? o.w : 0.f;
    }
    *reinterpret_cast<float4 *>(out + e[k] * ld_out + c) = o;
  }
}
}  // namespace
}  // namespace ptgnn_amd

extern "C" int ptgnn_amd_segment_spread_f32(const float *grad, int64_t ld_grad, const int32_t *arg,
                                            const int32_t *slot_row, const int32_t *perm,
                                            int64_t num_slots, int32_t dim, float *out, int64_t ld_out,
                                            void *stream_) {
  PTGNN_REQUIRE(num_slots >= 0 && dim > 0, PTGNN_AMD_EINVAL, "segment_spread: bad sizes");
  if (num_slots == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(grad && slot_row && perm && out, PTGNN_AMD_EINVAL, "segment_spread: null pointer");
  PTGNN_REQUIRE(ld_grad >= dim && ld_out >= dim, PTGNN_AMD_EINVAL, "segment_spread: bad leading dimension");
  const bool vec4 = (dim % 4 == 0) && (ld_grad % 4 == 0) && (ld_out % 4 == 0) && aligned16(grad) &&
                    aligned16(out) && (!arg || aligned16(arg));
  if (vec4 && (dim == 64 || dim == 128 || dim == 256) && num_slots < ((int64_t)1 << 31)) {
#ifndef PTGNN_SPREAD_SPG
#define PTGNN_SPREAD_SPG 2   // measured at [625 k, 128] max: 1 -> 112 us, 2 -> 92, 4 -> 95 (generic kernel: 120)
#endif
    constexpr int SPG = PTGNN_SPREAD_SPG;
    hipStream_t st = (hipStream_t)stream_;
#define PTGNN_SPREAD(LPRV)                                                                                     \
  do {                                                                                                         \
    const int64_t per_block = (256 / LPRV) * SPG;                                                              \
    const unsigned grid = (unsigned)((num_slots + per_block - 1) / per_block);                                 \
    if (arg) k_segment_spread_rows<LPRV, SPG, true><<<grid, 256, 0, st>>>(grad, ld_grad, arg, slot_row, perm, num_slots, out, ld_out); \
    else k_segment_spread_rows<LPRV, SPG, false><<<grid, 256, 0, st>>>(grad, ld_grad, arg, slot_row, perm, num_slots, out, ld_out);    \
  } while (0)
    if (dim == 64) PTGNN_SPREAD(16); else if (dim == 128) PTGNN_SPREAD(32); else PTGNN_SPREAD(64);
#undef PTGNN_SPREAD
    PTGNN_LAUNCH_CHECK();
    return PTGNN_AMD_OK;
  }
  const int64_t items = num_slots * (vec4 ? dim / 4 : dim);
  int64_t blocks = (items + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  if (vec4)
    k_segment_spread<true><<<(unsigned)blocks, 256, 0, (hipStream_t)stream_>>>(
        grad, ld_grad, arg, slot_row, perm, num_slots, dim, out, ld_out);
  else
    k_segment_spread<false><<<(unsigned)blocks, 256, 0, (hipStream_t)stream_>>>(
        grad, ld_grad, arg, slot_row, perm, num_slots, dim, out, ld_out);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}
