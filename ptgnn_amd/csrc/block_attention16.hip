// The 16-bit-input forward of the block self-attention (block_attention.hip; selfattmessagepassing.py:104-117 as an
// `enable_amp` user of the reference runs it: both einsums in the autocast dtype, the softmax in fp32).  Inference only:
// no dropout, no backward.  Same window table, same kqv [N, heads (2 dk + dv)] (fp32 in HBM, read in place), same fp32
// out / lse, and the same workgroup <-> (window, head, row block) map (block_attention.h) with 4 waves = 128 key rows.
//
// Operands.  Keys, queries and values are rounded to bf16 / fp16 (round to nearest even, gradual underflow: what
// tensor.to(dtype) does) when they are staged into LDS; the LDS tiles are 16-bit, d zero-padded to the MFMA's K step of
// 16.  Both products are v_mfma_f32_32x32x16_{bf16,f16} through half16.h's Half16<DT>:
//   * S^T[v, k] = sum_d Q[v, d] K[k, d]: A = the query tile, B = the wave's keys, both [row][d] images read as one
//     ds_read_b128 per lane and step (row l & 31, d = 16 s + 8 (l >> 5) ..).  The row stride is dk padded to 16, + 8
//     elements: an odd number of 16-byte units, so the reads of consecutive rows do not collide (half16.h).  The tile is
//     held transposed, lane = key row, as in the fp32 kernel: a row's softmax statistics live in one lane pair.
//   * scale, mask, running max and sum, exp, the accumulator rescale and the final division are fp32; l sums the
//     UNROUNDED probabilities; lse = m + log l.
//   * out[k, :] += sum_v P[k, v] V[v, :]: the unnormalised probabilities exp(S - m) are rounded in registers and ARE the A
//     operand -- registers 8 s .. 8 s + 7 of a lane half form the K-block of step s, i.e. the summed index runs over
//     the tile's rows ba_row(8 s + i, h).  The B operand reads exactly those rows of the [row][d] value image with two
//     transposed reads (ds_read_b64_tr_b16: rows 16 s + 4 h .. + 3 and 8 below, column 32 t + (l & 31)).  The value
//     image's row stride is 32 x odd elements: the four rows of a half's read start 16 banks apart (half16.h).
//
// Pipeline.  The walked query / value tile is double-buffered: the next tile's global loads are issued before the
// current tile's MFMAs and parked (rounded) into the other buffer after them, one barrier per tile.  The accumulator
// rescale is skipped when no row's maximum moved (alpha == 1 in every lane: multiplying by 1 changes no bit).
//
// Every sum runs in tile order inside one wave: no atomics, deterministic, and a window's result does not depend on
// where the window sits in the batch (alignment only chooses between one float4 load and four scalar loads of the
// same values).
#include "block_attention.h"
#include "half16.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

constexpr int kBa16Threads = 64 * kBaMaxWaves;
constexpr int kBa16Rows = kBaTile * kBaMaxWaves;   // key rows of a workgroup

// LDS row strides in 16-bit elements: keys / queries (row reads), values (transposed reads)
inline int ba16_ldk(int dk) { return (dk + 15) / 16 * 16 + 8; }
constexpr int ba16_ldv(int dvt) { return 32 * (dvt | 1); }

size_t ba16_lds_bytes(int dk, int dvt) {
  return sizeof(uint16_t) * ((size_t)(kBa16Rows + 2 * kBaTile) * ba16_ldk(dk) + (size_t)2 * kBaTile * ba16_ldv(dvt));
}

// columns c .. c + 3 of a row of `width` live columns (c % 4 == 0; columns past the width: 0).  `vec`: the row is 16-byte
// aligned and width % 4 == 0, so a live c has all four
__device__ __forceinline__ float4 ba16_load4(const float *__restrict__ row, int c, int width, bool vec) {
  if (vec) return c < width ? *reinterpret_cast<const float4 *>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = c < width ? row[c] : 0.f;
  v.y = c + 1 < width ? row[c + 1] : 0.f;
  v.z = c + 2 < width ? row[c + 2] : 0.f;
  v.w = c + 3 < width ? row[c + 3] : 0.f;
  return v;
}

// out[k, head dv + :] and lse[k, head] of the rows of one (window, head) row block
template <int DT, int DVT>
__global__ __launch_bounds__(kBa16Threads) void k_block_attention16(
    const float *__restrict__ kqv, int64_t ld, const int32_t *__restrict__ windows, BaShape sh, int vec,
    float *__restrict__ out, int64_t ld_out, float *__restrict__ lse) {
  using H = Half16<DT>;
  using vec8 = typename H::vec;
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = ((sh.dk + 15) >> 4) * 16 + 8, dkp = ldk - 8;
  constexpr int ldv = ba16_ldv(DVT);
  uint16_t *Ks = lds16, *Qs = Ks + kBa16Rows * ldk, *Vs = Qs + 2 * kBaTile * ldk;   // Qs, Vs: two buffers each
  const float *base = kqv + (int64_t)head * (2 * sh.dk + sh.dv);
  const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);   // a thread's float4 of a 32 x 32 staging block

  float4 qreg[4], vreg[DVT];
  auto fetch = [&](int j0) {       // the walked tile's rows -> registers
    int64_t g = (int64_t)start + j0 + srow;
    if (g >= end) g = end - 1;
    const float *row = base + g * ld;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < sh.dkt) qreg[t] = ba16_load4(row + sh.dk, 32 * t + scol, sh.dk, vec);
#pragma unroll
    for (int t = 0; t < DVT; ++t) vreg[t] = ba16_load4(row + 2 * sh.dk, 32 * t + scol, sh.dv, vec);
  };
  auto park = [&](int buf) {       // registers -> the rounded 16-bit tile
    uint16_t *q = Qs + buf * kBaTile * ldk + srow * ldk, *v = Vs + buf * kBaTile * ldv + srow * ldv;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < sh.dkt && 32 * t + scol < dkp) store4<DT>(q + 32 * t + scol, qreg[t]);
#pragma unroll
    for (int t = 0; t < DVT; ++t) store4<DT>(v + 32 * t + scol, vreg[t]);
  };

  fetch(0);
  for (int rb = 0; rb < kBaMaxWaves; ++rb) {       // the workgroup's own key rows, once
    int64_t g = (int64_t)start + r0 + kBaTile * rb + srow;
    if (g >= end) g = end - 1;
    const float *row = base + g * ld;
    uint16_t *k = Ks + (kBaTile * rb + srow) * ldk;
    for (int t = 0; t < sh.dkt; ++t)
      if (32 * t + scol < dkp) store4<DT>(k + 32 * t + scol, ba16_load4(row, 32 * t + scol, sh.dk, vec));
  }
  park(0);
  __syncthreads();

  const int wrow = r0 + kBaTile * wave;            // first row of the wave inside the window
  const bool live = wrow < n;                      // a wave without rows still stages and meets the barriers
  const int ksteps = dkp >> 4;
  const int64_t krow = (int64_t)start + wrow + c;  // the lane's key row (not stored when >= end)
  const uint16_t *Kw = Ks + (kBaTile * wave + c) * ldk + 8 * h;
  // this lane's address inside a 4-row x 16-column block of a transposed read (half16.h, tr8)
  const int tr_off = (4 * h + ((lane >> 2) & 3)) * ldv + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  f32x16 o[DVT];
#pragma unroll
  for (int t = 0; t < DVT; ++t) zero(o[t]);
  float m = -INFINITY, l = 0.0f;

  int cur = 0;
  for (int j0 = 0; j0 < n; j0 += kBaTile) {
    const bool more = j0 + kBaTile < n;
    if (more) fetch(j0 + kBaTile);
    if (live) {
      const uint16_t *Qb = Qs + cur * kBaTile * ldk + c * ldk + 8 * h;
      f32x16 x;                                             // S^T[v, k]: lane = key row, registers = queries
      zero(x);
      for (int s = 0; s < ksteps; ++s) x = H::mfma(load8<DT>(Qb + 16 * s), load8<DT>(Kw + 16 * s), x);
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        x[r] = j0 + ba_row(r, h) < n ? x[r] * sh.scale : -INFINITY;
        tmax = fmaxf(tmax, x[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mnew = fmaxf(m, tmax);                    // finite: column j0 is inside the window
      const float alpha = ba_exp(m - mnew);
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        x[r] = ba_exp(x[r] - mnew);
        psum += x[r];                                       // the unrounded probabilities
      }
      psum += __shfl_xor(psum, 32, 64);
      l = l * alpha + psum;
      m = mnew;
      if (__ballot(alpha != 1.0f)) {                        // some row's maximum moved
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = __shfl(alpha, ba_row(r, h), 64);  // the rescale of accumulator row r lives in that row's lane
#pragma unroll
          for (int t = 0; t < DVT; ++t) o[t][r] *= a;
        }
      }
      const uint16_t *Vb = Vs + cur * kBaTile * ldv + tr_off;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x8 pf = {x[8 * s], x[8 * s + 1], x[8 * s + 2], x[8 * s + 3],
                          x[8 * s + 4], x[8 * s + 5], x[8 * s + 6], x[8 * s + 7]};
        const vec8 p = __builtin_convertvector(pf, vec8);   // rows ba_row(8 s + i, h) of the tile, i = 0 .. 7
#pragma unroll
        for (int t = 0; t < DVT; ++t) {
          const uint16_t *at = Vb + 16 * s * ldv + 32 * t;
          o[t] = H::mfma(p, tr8<DT>(at, at + 8 * ldv), o[t]);
        }
      }
    }
    if (more) park(cur ^ 1);
    __syncthreads();                 // the other buffer is complete; everyone is done reading this one
    cur ^= 1;
  }
  if (!live) return;
  const float inv = 1.0f / l;
  if (h == 0 && wrow + c < n) lse[krow * sh.heads + head] = m + logf(l);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float a = __shfl(inv, ba_row(r, h), 64);
    const int row = wrow + ba_row(r, h);
    if (row < n) {
      float *dst = out + ((int64_t)start + row) * ld_out + (int64_t)head * sh.dv;
#pragma unroll
      for (int t = 0; t < DVT; ++t)
        if (32 * t + c < sh.dv) dst[32 * t + c] = o[t][r] * a;
    }
  }
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_attention16_block_supported(int32_t dk, int32_t dv, int32_t dtype) {
  return half16::dtype_ok(dtype) && dk >= 1 && dk <= kBaMaxDim && dv >= 1 && dv <= kBaMaxDim ? 1 : 0;
}

extern "C" int ptgnn_amd_attention16_block(const float *kqv, int64_t ld_kqv, const int32_t *windows,
                                           int64_t num_windows, int64_t num_rows, int32_t max_num_nodes,
                                           int32_t num_heads, int32_t dk, int32_t dv, float *out, int64_t ld_out,
                                           float *lse, int32_t dtype, void *stream_) {
  PTGNN_REQUIRE(half16::dtype_ok(dtype), PTGNN_AMD_EINVAL, "block_attention16: unknown dtype id %d", dtype);
  const int rc = ba_check("block_attention16", kqv, ld_kqv, windows, num_windows, num_rows, max_num_nodes, num_heads, dk,
                          dv, 0.0f);
  if (rc != PTGNN_AMD_OK || num_rows == 0) return rc;
  PTGNN_REQUIRE(out && lse, PTGNN_AMD_EINVAL, "block_attention16: null pointer");
  PTGNN_REQUIRE(ld_out >= (int64_t)num_heads * dv, PTGNN_AMD_EINVAL, "block_attention16: bad leading dimension");
  PTGNN_REQUIRE(half16::aligned4(kqv), PTGNN_AMD_EINVAL, "block_attention16: kqv is not 4-byte aligned");
  const int dvt = (dv + 31) / 32;
  const size_t bytes = ba16_lds_bytes(dk, dvt);
  const BaShape sh = ba_shape(num_heads, dk, dv, kBaMaxWaves, num_rows, max_num_nodes);
  PTGNN_REQUIRE(num_windows * sh.row_tiles < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "block_attention16: too many windows");
  // every float4 of a head's keys, queries and values is 16-byte aligned
  const int vec = half16::rows16(kqv, ld_kqv) && dk % 4 == 0 && dv % 4 == 0 ? 1 : 0;
  const dim3 grid((unsigned)(num_windows * sh.row_tiles), (unsigned)num_heads);
  hipStream_t st = (hipStream_t)stream_;
  int rc2 = PTGNN_AMD_OK;
  half16::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    BA_TILES(dvt, {
      auto kern = k_block_attention16<DT, TT>;
      if (!ba_lds_ok(kern, bytes)) {
        rc2 = PTGNN_AMD_EHIP;
        return;
      }
      kern<<<grid, kBa16Threads, bytes, st>>>(kqv, ld_kqv, windows, sh, vec, out, ld_out, lse);
    })
  });
  PTGNN_REQUIRE(rc2 == PTGNN_AMD_OK, PTGNN_AMD_EHIP, "block_attention16: %zu bytes of LDS refused", bytes);
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BLOCK_ATTENTION16);
  return PTGNN_AMD_OK;
}
