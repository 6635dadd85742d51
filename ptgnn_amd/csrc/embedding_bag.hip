// The subtoken pool of SubtokenUnitEmbedder (ptgnn/neuralmodels/embeddings/strelementrepresentationmodel.py:61-82), the
// node embedder every shipped model starts its forward with (graphneuralnetwork.py:160): row b of the output combines the
// table rows of the first lengths[b] of its S subtoken ids,
//     sum :  out[b] = sum_{s < len} table[ids[b, s]]                     (live rows added in slot order)
//     mean:  the sum / (float(lengths[b]) + 1e-10f)                      (the GIVEN length, also when it exceeds S)
//     max :  out[b, d] = max_{s < len} table[ids[b, s], d] from -inf,  arg[b, d] = the first slot that attains it (-1: none)
// The reference materialises embedded = table[ids] as [B, S, D], masks it (a read and a write), reduces it and keeps the
// 3-D tensor for autograd; here the ids (8 B per slot) and the table rows -- a 10 k x 128 vocabulary is 5 MB and stays in
// L2 -- are read and B * D floats are written.  Dead slots (s >= lengths[b]) are never read; ids are clamped into [0, V)
// before they address the table.
//
// Layout (HBM / L2-bound, no MFMA): one output row per group of LPR lanes, LPR = the power of two >= D / 4 up to a wave;
// a lane owns the float4 column chunks g, g + LPR, ... of its row (one at D <= 256), so a wave reads 1 KiB of table rows
// per load instruction and widths below 256 pack 64 / LPR rows into a wave (D = 4: 64 rows).  The slots of a row are
// walked in groups of 8: the ids of a group are loaded first, then all of its row loads are issued before the first use
// (S = 5, the reference's max_num_subtokens: every table read of a row is in flight together) and folded in slot order.
// 256-thread workgroups, 64 (sum) to 78 (max) VGPRs, no LDS, no scratch: six to eight waves per SIMD stay resident to hide
// the dependent id -> row round trip.
//
// Backward: the bag is a one-edge-type graph -- element e = b * S + s has source b and destination ids[e] -- so the table
// gradient is a segment sum over the stable destination-sorted plan of those elements (ptgnn_amd_csr_build, mode 0):
// ptgnn_amd_embedding_bag_keys writes the (source, key) pairs with the key of a DEAD slot set to V, one past the last
// vocabulary row, and the walk covers the rows [0, V) only, so padding costs no gather and nobody reads sum(lengths)
// back.  The walk is gather_reduce_core.h's: rows in slot order (= element order), rows beyond 256 elements in their
// own launch, beyond the hub threshold in 1024-slot chunks folded in chunk order -- the order depends on the ids, never
// on the launch geometry; integer tickets only, no float atomics.  mean pre-scales the gradient rows by 1 / (len + 1e-10f);
// max routes g[b, d] to slot arg[b, d] through the arg-routed reduce of the max / min aggregation.  A vocabulary row nobody
// references is an empty segment: exactly 0.
//
// Supported: D % 4 == 0, 4 <= D <= 1024, 1 <= S <= 32; other shapes answer PTGNN_AMD_EUNSUPPORTED and the host composes
// the reference's operator sequence from the row gather.
#include <math.h>

#include "common.h"

namespace ptgnn_amd {
namespace {

constexpr int kBagThreads = 256;
constexpr int kBagGroup = 8;       // slots whose table rows are in flight together
constexpr int kBagMaxSlots = 32;
constexpr int kBagMaxDim = 1024;

bool bag_supported(int dim, int slots) {
  return dim >= 4 && dim <= kBagMaxDim && dim % 4 == 0 && slots >= 1 && slots <= kBagMaxSlots;
}

// log2 of the lanes per row: the power of two >= dim / 4, at most a wave
int bag_lane_shift(int dim) {
  int shift = 0;
  while ((1 << shift) < dim / 4 && shift < 6) ++shift;
  return shift;
}

template <int MODE>
__global__ __launch_bounds__(kBagThreads) void k_embedding_bag(
    const float *__restrict__ table, int64_t ld_table, int64_t vocab, const int64_t *__restrict__ ids,
    const int64_t *__restrict__ lengths, int64_t num_bags, int slots, int dim, int lane_shift, float *__restrict__ out,
    int64_t ld_out, int32_t *__restrict__ arg) {
  const int lpr = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBagThreads >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= num_bags) return;          // a whole lane group leaves together; there is no cross-lane step
  const int g = threadIdx.x & (lpr - 1);
  const int64_t given = lengths[b];
  const int live = given < 0 ? 0 : (given < slots ? (int)given : slots);
  const int64_t *row_ids = ids + b * slots;
  for (int q = g; 4 * q < dim; q += lpr) {
    float acc[4];
    int win[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) { acc[v] = MODE == PTGNN_AMD_MAX ? -INFINITY : 0.0f; win[v] = -1; }
    for (int s0 = 0; s0 < live; s0 += kBagGroup) {
      int64_t id[kBagGroup];
#pragma unroll
      for (int j = 0; j < kBagGroup; ++j) {
        id[j] = 0;
        if (s0 + j < live) {
          const int64_t t = row_ids[s0 + j];
          id[j] = t < 0 ? 0 : (t < vocab ? t : vocab - 1);
        }
      }
      float4 r[kBagGroup];
#pragma unroll
      for (int j = 0; j < kBagGroup; ++j)
        if (s0 + j < live) r[j] = *reinterpret_cast<const float4 *>(table + id[j] * ld_table + 4 * q);
#pragma unroll
      for (int j = 0; j < kBagGroup; ++j)
        if (s0 + j < live) {
          const float m[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (MODE == PTGNN_AMD_MAX) {
              if (m[v] > acc[v] || m[v] != m[v]) { acc[v] = m[v]; win[v] = s0 + j; }   // ties keep the first slot; NaN stays
            } else {
              acc[v] += m[v];
            }
          }
        }
    }
    if (MODE == PTGNN_AMD_MEAN) {
      const float div = (float)given + 1e-10f;
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[v] = acc[v] / div;
    }
    *reinterpret_cast<float4 *>(out + b * ld_out + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    if (MODE == PTGNN_AMD_MAX && arg)
      *reinterpret_cast<int4 *>(arg + b * (int64_t)dim + 4 * q) = make_int4(win[0], win[1], win[2], win[3]);
  }
}

// element e = b * S + s of the bag as an edge: source b, destination ids[e] clamped into [0, V), V for a dead slot
__global__ __launch_bounds__(256) void k_bag_keys(const int64_t *__restrict__ ids, const int64_t *__restrict__ lengths,
                                                   int64_t num_elements, int slots, int64_t vocab,
                                                   int64_t *__restrict__ src, int64_t *__restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_elements) return;
  const int64_t b = e / slots;
  const int s = (int)(e - b * slots);
  const int64_t t = ids[e];
  src[e] = b;
  key[e] = s < lengths[b] ? (t < 0 ? 0 : (t < vocab ? t : vocab - 1)) : vocab;
}

// scaled[b, :] = grad[b, :] / (float(lengths[b]) + 1e-10f): the mean's divisor, applied once per gradient row
__global__ __launch_bounds__(256) void k_bag_scale(const float *__restrict__ grad, int64_t ld_grad,
                                                    const int64_t *__restrict__ lengths, int64_t num_bags, int dim,
                                                    float *__restrict__ scaled) {
  const int per_row = dim / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_bags * per_row) return;
  const int64_t b = i / per_row;
  const int q = (int)(i - b * per_row);
  const float div = (float)lengths[b] + 1e-10f;
  const float4 gv = *reinterpret_cast<const float4 *>(grad + b * ld_grad + 4 * q);
  *reinterpret_cast<float4 *>(scaled + b * (int64_t)dim + 4 * q) = make_float4(gv.x / div, gv.y / div, gv.z / div, gv.w / div);
}

// slot_of[i] = the bag slot s of the element in plan slot i (element perm[i] = b * S + s)
__global__ __launch_bounds__(256) void k_bag_slots(const int32_t *__restrict__ perm, int64_t num_elements, int slots,
                                                    int32_t *__restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < num_elements) slot_of[i] = perm[i] % slots;
}

// the checks every entry point shares; 0 when the sizes are fine
int bag_check(const char *what, int64_t num_bags, int32_t slots, int64_t vocab, int32_t dim, int mode) {
  PTGNN_REQUIRE(num_bags >= 0 && vocab >= 0 && slots > 0 && dim > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(mode >= PTGNN_AMD_SUM && mode <= PTGNN_AMD_MAX, PTGNN_AMD_EINVAL, "%s: mode %d is not sum / mean / max",
                what, mode);
  PTGNN_REQUIRE(bag_supported(dim, slots), PTGNN_AMD_EUNSUPPORTED,
                "%s: dim %d / %d slots outside the kernel range (dim %% 4 == 0, 4 <= dim <= %d, slots <= %d)", what, dim,
                slots, kBagMaxDim, kBagMaxSlots);
  PTGNN_REQUIRE(num_bags <= (((int64_t)1 << 31) - 1) / slots && vocab < ((int64_t)1 << 31) - 1, PTGNN_AMD_EUNSUPPORTED,
                "%s: too many bags / vocabulary rows", what);
  return PTGNN_AMD_OK;
}

size_t bag_backward_workspace(int64_t num_bags, int32_t slots, int32_t dim, int mode) {
  if (mode == PTGNN_AMD_MEAN) return (size_t)num_bags * dim * sizeof(float);
  if (mode == PTGNN_AMD_MAX) return (size_t)num_bags * slots * sizeof(int32_t);
  return 0;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_embedding_bag_supported(int32_t dim, int32_t slots) { return bag_supported(dim, slots) ? 1 : 0; }

extern "C" int ptgnn_amd_embedding_bag_f32(const float *table, int64_t ld_table, int64_t vocab, const int64_t *ids,
                                           const int64_t *lengths, int64_t num_bags, int32_t slots, int32_t dim, int mode,
                                           float *out, int64_t ld_out, int32_t *arg, void *stream_) {
  if (const int rc = bag_check("embedding_bag", num_bags, slots, vocab, dim, mode)) return rc;
  if (num_bags == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(table && ids && lengths && out && vocab > 0, PTGNN_AMD_EINVAL, "embedding_bag: null pointer / empty table");
  PTGNN_REQUIRE(ld_table >= dim && ld_out >= dim, PTGNN_AMD_EINVAL, "embedding_bag: bad leading dimension");
  PTGNN_REQUIRE(arg == nullptr || mode == PTGNN_AMD_MAX, PTGNN_AMD_EINVAL, "embedding_bag: arg only with max");
  PTGNN_REQUIRE(ld_table % 4 == 0 && ld_out % 4 == 0 && aligned16(table) && aligned16(out) && aligned16(arg),
                PTGNN_AMD_EUNSUPPORTED, "embedding_bag: rows must be 16-byte aligned");
  const int shift = bag_lane_shift(dim);
  const int64_t rows_per_block = kBagThreads >> shift;
  const unsigned grid = (unsigned)((num_bags + rows_per_block - 1) / rows_per_block);
  hipStream_t st = (hipStream_t)stream_;
  switch (mode) {
    case PTGNN_AMD_SUM:
      k_embedding_bag<PTGNN_AMD_SUM><<<grid, kBagThreads, 0, st>>>(table, ld_table, vocab, ids, lengths, num_bags, slots,
                                                                   dim, shift, out, ld_out, arg);
      break;
    case PTGNN_AMD_MEAN:
      k_embedding_bag<PTGNN_AMD_MEAN><<<grid, kBagThreads, 0, st>>>(table, ld_table, vocab, ids, lengths, num_bags, slots,
                                                                    dim, shift, out, ld_out, arg);
      break;
    default:
      k_embedding_bag<PTGNN_AMD_MAX><<<grid, kBagThreads, 0, st>>>(table, ld_table, vocab, ids, lengths, num_bags, slots,
                                                                   dim, shift, out, ld_out, arg);
      break;
  }
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_EMBEDDING_BAG);
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_embedding_bag_keys(const int64_t *ids, const int64_t *lengths, int64_t num_bags, int32_t slots,
                                            int64_t vocab, int64_t *src, int64_t *key, void *stream_) {
  PTGNN_REQUIRE(num_bags >= 0 && vocab >= 0 && slots > 0, PTGNN_AMD_EINVAL, "embedding_bag_keys: bad sizes");
  PTGNN_REQUIRE(slots <= kBagMaxSlots, PTGNN_AMD_EUNSUPPORTED, "embedding_bag_keys: %d slots outside the kernel range (<= %d)",
                slots, kBagMaxSlots);
  PTGNN_REQUIRE(num_bags <= (((int64_t)1 << 31) - 1) / slots && vocab < ((int64_t)1 << 31) - 1, PTGNN_AMD_EUNSUPPORTED,
                "embedding_bag_keys: too many bags / vocabulary rows");
  if (num_bags == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(ids && lengths && src && key && vocab > 0, PTGNN_AMD_EINVAL, "embedding_bag_keys: null pointer / empty table");
  const int64_t n = num_bags * slots;
  k_bag_keys<<<blocks_of(n), 256, 0, (hipStream_t)stream_>>>(ids, lengths, n, slots, vocab, src, key);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_embedding_bag_backward_workspace_bytes(int64_t num_bags, int32_t slots, int32_t dim, int mode) {
  if (num_bags <= 0 || slots <= 0 || dim <= 0) return 0;
  return bag_backward_workspace(num_bags, slots, dim, mode);
}

extern "C" int ptgnn_amd_embedding_bag_backward_f32(const float *grad, int64_t ld_grad, const int64_t *lengths,
                                                    const int32_t *arg, int64_t num_bags, int32_t slots, int64_t vocab,
                                                    int32_t dim, int mode, const int32_t *rowptr, const int32_t *col,
                                                    const int32_t *perm, float *grad_table, int64_t ld_gt,
                                                    int32_t hub_threshold, const int32_t *hub_entries,
                                                    const int32_t *hub_count, void *hub_ws, size_t hub_ws_bytes,
                                                    int32_t *hub_tickets, void *workspace, size_t workspace_bytes,
                                                    void *stream_) {
  if (const int rc = bag_check("embedding_bag_backward", num_bags, slots, vocab, dim, mode)) return rc;
  if (vocab == 0) return PTGNN_AMD_OK;
  PTGNN_REQUIRE(rowptr && col && grad_table && (num_bags == 0 || (grad && lengths)), PTGNN_AMD_EINVAL,
                "embedding_bag_backward: null pointer");
  PTGNN_REQUIRE(mode != PTGNN_AMD_MAX || num_bags == 0 || (arg && perm), PTGNN_AMD_EINVAL,
                "embedding_bag_backward: max needs the forward's arg and the plan's perm");
  PTGNN_REQUIRE(ld_gt >= dim && (num_bags == 0 || ld_grad >= dim), PTGNN_AMD_EINVAL,
                "embedding_bag_backward: bad leading dimension");
  PTGNN_REQUIRE(ld_gt % 4 == 0 && ld_grad % 4 == 0 && aligned16(grad) && aligned16(grad_table) && aligned16(arg) &&
                    aligned16(workspace),
                PTGNN_AMD_EUNSUPPORTED, "embedding_bag_backward: rows must be 16-byte aligned");
  const size_t need = bag_backward_workspace(num_bags, slots, dim, mode);
  PTGNN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), PTGNN_AMD_EWORKSPACE,
                "embedding_bag_backward: workspace of %zu bytes, need %zu", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream_;
  const int64_t elements = num_bags * slots;
  int rc;
  if (mode == PTGNN_AMD_MAX && num_bags > 0) {
    int32_t *slot_of = static_cast<int32_t *>(workspace);
    k_bag_slots<<<blocks_of(elements), 256, 0, st>>>(perm, elements, slots, slot_of);
    PTGNN_LAUNCH_CHECK();
    // rows [0, vocab) of the plan: the dead slots' row `vocab` is never walked
    rc = ptgnn_amd_gather_reduce_masked_f32(grad, ld_grad, arg, rowptr, col, slot_of, vocab, dim, grad_table, ld_gt,
                                            elements, hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes,
                                            hub_tickets, stream_);
  } else {
    const float *rows = grad;
    int64_t ld_rows = ld_grad;
    if (mode == PTGNN_AMD_MEAN && num_bags > 0) {
      float *scaled = static_cast<float *>(workspace);
      k_bag_scale<<<blocks_of(num_bags * (dim / 4)), 256, 0, st>>>(grad, ld_grad, lengths, num_bags, dim, scaled);
      PTGNN_LAUNCH_CHECK();
      rows = scaled;
      ld_rows = dim;
    }
    rc = ptgnn_amd_gather_reduce_rows_f32(rows, ld_rows, nullptr, ld_rows, rowptr, col, 0, vocab + 1, dim, PTGNN_AMD_SUM,
                                          PTGNN_AMD_EPI_NONE, nullptr, nullptr, 0.0f, grad_table, ld_gt, nullptr, elements,
                                          hub_threshold, hub_entries, hub_count, hub_ws, hub_ws_bytes, hub_tickets, 0,
                                          vocab, stream_);
  }
  if (rc != PTGNN_AMD_OK) return rc;
  count_launch(PTGNN_AMD_KERNEL_EMBEDDING_BAG_BACKWARD);
  return PTGNN_AMD_OK;
}
