// EGC-S head / basis combination (egcmessagepassing.py:63-91): per node v with K heads, B bases, Dh = D / K,
//     out[v, k*Dh + d] = sum_b  w[v, k*B + b] * agg[v, k*B*Dh + b*Dh + d]
// Contract: include/ptgnn_amd.h (ptgnn_amd_egc_*).
//
//   * ptgnn_amd_egc_gather_combine_f32: the CSR aggregation of gather_reduce_core.h (same row walk, hub chunks, long
//     rows, fold order and arg) with the combine as the row finish (RowOp::combine_store): inference never writes the
//     [N, B*D] aggregate.  Training asks for it (and the max / min arg) through the nullable agg_out / argout.
//   * ptgnn_amd_egc_combine_f32 / _backward_f32: the combine alone and its one-pass backward
//         g_agg[v, k,b,d] = w[v,k,b] * g[v,k,d]        g_w[v, k,b] = sum_d agg[v,k,b,d] * g[v,k,d]
//     for any (K, B, Dh): a float4 form where Dh % 4 == 0 (the backward's g_w dot product then reduces over the
//     Dh/4 lanes of a (k, b) with shuffles, so Dh/4 must be a power of two) and a scalar form for everything else.
// Algorithmic bytes (backward): read agg 4*B*D + g 4*D + w 4*K*B, write g_agg 4*B*D + g_w 4*K*B per node.
#include "gather_reduce_core.h"

namespace ptgnn_amd {
namespace {

template <int VEC, int LPR, int CH>
int launch_combined(const Args &a, int reduce, hipStream_t s) {
  switch (reduce) {
    case PTGNN_AMD_SUM:
      return launch_all<VEC, LPR, CH, PTGNN_AMD_SUM, false, false, false, true>(a, 1, s);
    case PTGNN_AMD_MEAN:
      return launch_all<VEC, LPR, CH, PTGNN_AMD_MEAN, false, false, false, true>(a, 1, s);
    case PTGNN_AMD_MAX:
      return a.argout ? launch_all<VEC, LPR, CH, PTGNN_AMD_MAX, false, true, false, true>(a, 1, s)
                      : launch_all<VEC, LPR, CH, PTGNN_AMD_MAX, false, false, false, true>(a, 1, s);
    default:
      return a.argout ? launch_all<VEC, LPR, CH, PTGNN_AMD_MIN, false, true, false, true>(a, 1, s)
                      : launch_all<VEC, LPR, CH, PTGNN_AMD_MIN, false, false, false, true>(a, 1, s);
  }
}

// one thread per output quad (VEC4) or element; b folds in order, as in RowOp::combine_store (same bits)
template <bool VEC4>
__global__ __launch_bounds__(256) void k_egc_combine(const float *__restrict__ agg, int64_t ld_agg,
                                                     const float *__restrict__ coef, int64_t ld_coef, int64_t num_rows,
                                                     int K, int B, int Dh, float *__restrict__ out, int64_t ld_out) {
  const int per_row = VEC4 ? K * Dh / 4 : K * Dh;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_rows * per_row) return;
  const int64_t row = i / per_row;
  const int j = (int)(i - row * per_row) * (VEC4 ? 4 : 1);
  const int k = j / Dh, d = j - k * Dh;
  const float *cw = coef + row * ld_coef + k * B;
  const float *base = agg + row * ld_agg + k * B * Dh + d;
  if constexpr (VEC4) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
      const float w = cw[b];
      const float4 t = *reinterpret_cast<const float4 *>(base + b * Dh);
      s.x += w * t.x; s.y += w * t.y; s.z += w * t.z; s.w += w * t.w;
    }
    *reinterpret_cast<float4 *>(out + row * ld_out + j) = s;
  } else {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += cw[b] * base[b * Dh];
    out[row * ld_out + j] = s;
  }
}

// float4 backward: one thread per agg quad (v, k, b, d..d+3); the P = Dh/4 consecutive lanes of one (v, k, b) reduce
// their partial dot products with xor shuffles (P | 64 and P | K*B*P: a group never straddles a wave).  No early
// return before the shuffles: lanes past the end contribute zeros.
template <int P>
__global__ __launch_bounds__(256) void k_egc_combine_bwd4(const float *__restrict__ agg, int64_t ld_agg,
                                                          const float *__restrict__ coef, int64_t ld_coef,
                                                          const float *__restrict__ grad, int64_t ld_grad,
                                                          int64_t num_rows, int K, int B,
                                                          float *__restrict__ gagg, int64_t ld_gagg,
                                                          float *__restrict__ gcoef, int64_t ld_gcoef) {
  constexpr int Dh = 4 * P;
  const int per_row = K * B * P;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < num_rows * per_row;
  float p = 0.f;
  int64_t row = 0;
  int kb = 0, dq = 0;
  if (valid) {
    row = i / per_row;
    const int r = (int)(i - row * per_row);
    kb = r / P;
    dq = r - kb * P;
    const int k = kb / B;
    const float w = coef[row * ld_coef + kb];
    const float4 g = *reinterpret_cast<const float4 *>(grad + row * ld_grad + k * Dh + 4 * dq);
    const float4 a = *reinterpret_cast<const float4 *>(agg + row * ld_agg + (int64_t)kb * Dh + 4 * dq);
    *reinterpret_cast<float4 *>(gagg + row * ld_gagg + (int64_t)kb * Dh + 4 * dq) =
        make_float4(w * g.x, w * g.y, w * g.z, w * g.w);
    p = a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
  }
  p = group_sum<P>(p);
  if (valid && dq == 0) gcoef[row * ld_gcoef + kb] = p;
}

// scalar backward (any Dh): one thread per (v, k, b), d in order
__global__ __launch_bounds__(256) void k_egc_combine_bwd1(const float *__restrict__ agg, int64_t ld_agg,
                                                          const float *__restrict__ coef, int64_t ld_coef,
                                                          const float *__restrict__ grad, int64_t ld_grad,
                                                          int64_t num_rows, int K, int B, int Dh,
                                                          float *__restrict__ gagg, int64_t ld_gagg,
                                                          float *__restrict__ gcoef, int64_t ld_gcoef) {
  const int per_row = K * B;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_rows * per_row) return;
  const int64_t row = i / per_row;
  const int kb = (int)(i - row * per_row), k = kb / B;
  const float w = coef[row * ld_coef + kb];
  const float *g = grad + row * ld_grad + k * Dh;
  const float *a = agg + row * ld_agg + (int64_t)kb * Dh;
  float *ga = gagg + row * ld_gagg + (int64_t)kb * Dh;
  float p = 0.f;
  for (int d = 0; d < Dh; ++d) {
    ga[d] = w * g[d];
    p += a[d] * g[d];
  }
  gcoef[row * ld_gcoef + kb] = p;
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + 255) / 256); }

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_egc_gather_combine_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr,
                                                const int32_t *col, int32_t type_bits, int64_t num_nodes,
                                                int32_t num_heads, int32_t num_bases, int32_t head_dim, int reduce,
                                                const float *coef, int64_t ld_coef, float *out, int64_t ld_out,
                                                float *agg_out, int32_t *argout, int64_t num_edges,
                                                int32_t hub_threshold, const int32_t *hub_entries,
                                                const int32_t *hub_count, void *hub_ws, size_t hub_ws_bytes,
                                                int32_t *hub_tickets, void *stream_) {
  PTGNN_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_heads > 0 && num_bases > 0 && head_dim > 0, PTGNN_AMD_EINVAL,
                "egc_gather_combine: bad sizes");
  PTGNN_REQUIRE(reduce >= PTGNN_AMD_SUM && reduce <= PTGNN_AMD_MIN, PTGNN_AMD_EINVAL,
                "egc_gather_combine: unknown reduce %d", reduce);
  PTGNN_REQUIRE(type_bits >= 0 && type_bits < 16, PTGNN_AMD_EINVAL, "egc_gather_combine: bad type_bits");
  PTGNN_REQUIRE(argout == nullptr || (reduce >= PTGNN_AMD_MAX && agg_out != nullptr), PTGNN_AMD_EINVAL,
                "egc_gather_combine: argout only with max/min and together with agg_out");
  const int64_t m64 = (int64_t)num_heads * num_bases * head_dim;
  PTGNN_REQUIRE(m64 < (1 << 20), PTGNN_AMD_EINVAL, "egc_gather_combine: message width too large");
  const int32_t msg_dim = (int32_t)m64;
  const int32_t D = num_heads * head_dim;
  if (num_nodes == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && coef && out && (msg || num_edges == 0), PTGNN_AMD_EINVAL,
                "egc_gather_combine: null pointer");
  PTGNN_REQUIRE(ld_out >= D && ld_coef >= num_heads * num_bases && ld_msg >= msg_dim, PTGNN_AMD_EINVAL,
                "egc_gather_combine: bad leading dimension");
  const bool vec4 = (msg_dim % 4 == 0) && (ld_msg % 4 == 0) && aligned16(msg) && (!agg_out || aligned16(agg_out)) &&
                    (!argout || aligned16(argout));
  // the combine reads the whole row from one lane group: one column block (512 floats on the float4 path, 256 else)
  PTGNN_REQUIRE(msg_dim <= (vec4 ? 512 : 256), PTGNN_AMD_EUNSUPPORTED,
                "egc_gather_combine: heads*bases*head_dim = %d exceeds the fused kernel's row (%d); use "
                "gather_reduce + egc_combine", msg_dim, vec4 ? 512 : 256);
  Args a{};
  a.ysrc = msg; a.ydst = nullptr; a.ld_y = ld_msg; a.ld_yd = ld_msg;
  a.rowptr = rowptr; a.col = col; a.type_bits = type_bits; a.num_nodes = num_nodes; a.row_begin = 0; a.msg_dim = msg_dim;
  a.out = agg_out; a.ld_out = msg_dim; a.argout = argout; a.epi = 0;
  a.coef = coef; a.ld_coef = ld_coef; a.comb_out = out; a.ld_comb = ld_out;
  a.comb_heads = num_heads; a.comb_bases = num_bases; a.comb_dh = head_dim;
  a.comb_vec4 = (head_dim % 4 == 0) && (ld_out % 4 == 0) && aligned16(out);
  const int rc = setup_hub(a, num_edges, hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes, hub_tickets,
                           argout != nullptr);
  if (rc != PTGNN_AMD_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int rc2 = dispatch_geometry(vec4, msg_dim, false, [&](auto V, auto L, auto C, int col_blocks) {
    (void)col_blocks;   // 1: msg_dim is within one column block (checked above)
    return launch_combined<decltype(V)::value, decltype(L)::value, decltype(C)::value>(a, reduce, stream);
  });
  if (rc2 == PTGNN_AMD_OK) count_launch(PTGNN_AMD_KERNEL_EGC_GATHER_COMBINE);
  return rc2;
}

extern "C" int ptgnn_amd_egc_combine_f32(const float *agg, int64_t ld_agg, const float *coef, int64_t ld_coef,
                                         int64_t num_rows, int32_t num_heads, int32_t num_bases, int32_t head_dim,
                                         float *out, int64_t ld_out, void *stream_) {
  PTGNN_REQUIRE(num_rows >= 0 && num_heads > 0 && num_bases > 0 && head_dim > 0, PTGNN_AMD_EINVAL,
                "egc_combine: bad sizes");
  const int64_t D = (int64_t)num_heads * head_dim, KB = (int64_t)num_heads * num_bases;
  PTGNN_REQUIRE(KB * head_dim < (1 << 24), PTGNN_AMD_EINVAL, "egc_combine: row too wide");
  if (num_rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(agg && coef && out, PTGNN_AMD_EINVAL, "egc_combine: null pointer");
  PTGNN_REQUIRE(ld_agg >= KB * head_dim && ld_coef >= KB && ld_out >= D, PTGNN_AMD_EINVAL,
                "egc_combine: bad leading dimension");
  const bool vec4 = head_dim % 4 == 0 && ld_agg % 4 == 0 && ld_out % 4 == 0 && aligned16(agg) && aligned16(out);
  const int64_t items = num_rows * (vec4 ? D / 4 : D);
  PTGNN_REQUIRE(items / 256 < ((int64_t)1 << 31), PTGNN_AMD_EINVAL, "egc_combine: too many rows for one launch");
  hipStream_t st = (hipStream_t)stream_;
  if (vec4)
    k_egc_combine<true><<<blocks_for(items), 256, 0, st>>>(agg, ld_agg, coef, ld_coef, num_rows, num_heads, num_bases,
                                                           head_dim, out, ld_out);
  else
    k_egc_combine<false><<<blocks_for(items), 256, 0, st>>>(agg, ld_agg, coef, ld_coef, num_rows, num_heads,
                                                            num_bases, head_dim, out, ld_out);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_EGC_COMBINE);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_egc_combine_backward_f32(const float *agg, int64_t ld_agg, const float *coef, int64_t ld_coef,
                                                  const float *grad, int64_t ld_grad, int64_t num_rows,
                                                  int32_t num_heads, int32_t num_bases, int32_t head_dim,
                                                  float *grad_agg, int64_t ld_grad_agg, float *grad_coef,
                                                  int64_t ld_grad_coef, void *stream_) {
  PTGNN_REQUIRE(num_rows >= 0 && num_heads > 0 && num_bases > 0 && head_dim > 0, PTGNN_AMD_EINVAL,
                "egc_combine_backward: bad sizes");
  const int64_t D = (int64_t)num_heads * head_dim, KB = (int64_t)num_heads * num_bases;
  PTGNN_REQUIRE(KB * head_dim < (1 << 24), PTGNN_AMD_EINVAL, "egc_combine_backward: row too wide");
  if (num_rows == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(agg && coef && grad && grad_agg && grad_coef, PTGNN_AMD_EINVAL, "egc_combine_backward: null pointer");
  PTGNN_REQUIRE(ld_agg >= KB * head_dim && ld_coef >= KB && ld_grad >= D && ld_grad_agg >= KB * head_dim &&
                    ld_grad_coef >= KB,
                PTGNN_AMD_EINVAL, "egc_combine_backward: bad leading dimension");
  const int P = head_dim / 4;
  const bool vec4 = head_dim % 4 == 0 && (P & (P - 1)) == 0 && P <= 16 && ld_agg % 4 == 0 && ld_grad % 4 == 0 &&
                    ld_grad_agg % 4 == 0 && aligned16(agg) && aligned16(grad) && aligned16(grad_agg);
  hipStream_t st = (hipStream_t)stream_;
  if (vec4) {
    const int64_t items = num_rows * KB * P;
    PTGNN_REQUIRE(items / 256 < ((int64_t)1 << 31), PTGNN_AMD_EINVAL, "egc_combine_backward: too many rows");
#define PTGNN_EGC_BWD4(PV)                                                                                        \
  k_egc_combine_bwd4<PV><<<blocks_for(items), 256, 0, st>>>(agg, ld_agg, coef, ld_coef, grad, ld_grad, num_rows, \
                                                             num_heads, num_bases, grad_agg, ld_grad_agg,         \
                                                             grad_coef, ld_grad_coef)
    switch (P) {
      case 1: PTGNN_EGC_BWD4(1); break;
      case 2: PTGNN_EGC_BWD4(2); break;
      case 4: PTGNN_EGC_BWD4(4); break;
      case 8: PTGNN_EGC_BWD4(8); break;
      default: PTGNN_EGC_BWD4(16); break;
    }
#undef PTGNN_EGC_BWD4
  } else {
    const int64_t items = num_rows * KB;
    PTGNN_REQUIRE(items / 256 < ((int64_t)1 << 31), PTGNN_AMD_EINVAL, "egc_combine_backward: too many rows");
    k_egc_combine_bwd1<<<blocks_for(items), 256, 0, st>>>(agg, ld_agg, coef, ld_coef, grad, ld_grad, num_rows,
                                                          num_heads, num_bases, head_dim, grad_agg, ld_grad_agg,
                                                          grad_coef, ld_grad_coef);
  }
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_EGC_COMBINE_BACKWARD);
  return PTGNN_AMD_OK;
}
