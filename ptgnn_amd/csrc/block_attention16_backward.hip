// The 16-bit-input backward of the block self-attention (block_attention16.hip is its forward; block_attention.hip the
// exact-fp32 pair).  What autocast gives an `enable_amp` user of the reference for selfattmessagepassing.py:104-117: the
// four products of the backward in the 16-bit type, everything else fp32.  With P = exp(scale S - lse), M the dropout
// multiplier, D_k = sum_d dOut[k, d] out[k, d] (fp32 on the unrounded operands: k_block_attention_rowdot) and
// dS = P o (M o dP - D), all fp32,
//
//     d key_k   = scale sum_v rnd(dS[k, v]) rnd(query_v)      k_attention16_dkey: workgroup owns 128 key rows
//     d query_v = scale sum_k rnd(dS[k, v]) rnd(key_k)        k_attention16_dqv:  workgroup owns 128 query rows
//     d value_v = sum_k rnd((M o P)[k, v]) rnd(dOut_k)
//
// with S and dP = dOut V^T recomputed per tile pair from the rounded keys, queries, values and dOut rows.  Same window
// table, same workgroup <-> (window, head, row block) map (ba_locate, ba_shape, 4 waves x 32 rows), kqv / out / lse /
// grad_out fp32 in HBM and read in place, grad_kqv fp32.
//
// Products (v_mfma_f32_32x32x16_{bf16,f16} through half16.h's Half16<DT>), per walked tile of 32 rows:
//   * the two score products are row-read ones (A = the walked tile, B = the wave's own rows, both [row][d] images, one
//     ds_read_b128 per lane and k-step): the key kernel holds S^T[v, k] and dP^T[v, k] with lane = key row -- lse_k and
//     D_k live in the lane --, the query / value kernel S[k, v] and dP[k, v] with lane = query row, the tile's 32 lse
//     and D values beside it in LDS.
//   * dS (and M o P) are formed in fp32 in the accumulator registers, rounded ONCE, and ARE the A operand of the
//     gradient products: registers 8 s .. 8 s + 7 are the K-block of step s (ba16_round8), and the B operand reads the
//     same rows of the walked tile transposed (ds_read_b64_tr_b16) -- nothing goes back through LDS.
//   * a walked tile that is read both ways (the queries in the key kernel; the keys and dOut in the other) is parked as
//     two images, one per conflict-free stride (block_attention16.h says why there is no common one).
//
// LDS in 16-bit elements, ld(d) = d padded to 16, + 8; lt(T) = 32 (T | 1):
//   dkey: own K 128 ld(dk) + dOut 128 ld(dv); walked, two buffers each: Q rows 32 ld(dk), Q transposed 32 lt(DKT),
//         V rows 32 ld(dv).                                                 dk = dv = 128: 124 928 bytes
//   dqv:  own Q 128 ld(dk) + V 128 ld(dv); walked, two buffers each: K rows + K transposed, dOut rows + dOut
//         transposed, and 64 floats (lse, D).                               dk = dv = 128: 145 920 bytes
// Both fit the 160 KiB of a gfx950 workgroup with all 4 waves at every width up to 128, so there is no 2- or 1-wave
// form; beyond 64 KiB the limit is raised per kernel (ba_lds_ok).
//
// Pipeline as in the forward: the next tile's global loads are issued before the current tile's MFMAs and parked
// (rounded) into the other buffer after them, one barrier per tile.  Every sum runs in tile order inside one wave: no
// atomics, deterministic, and a window's gradients do not depend on where the window sits in the batch.  Nothing is
// clamped: a rounded dS or probability may underflow gradually and a rounded gradient may overflow to inf in fp16, as
// tensor.half() gives and GradScaler expects.
#include "block_attention16.h"

namespace ptgnn_amd {
namespace {

using namespace half16;

size_t ba16_dkey_lds_bytes(int dk, int dv, int dkt) {
  const size_t ldk = ba16_ldk(dk), ldg = ba16_ldk(dv);
  return sizeof(uint16_t) * (kBa16Rows * (ldk + ldg) + 2 * kBaTile * (ldk + ba16_ldv(dkt) + ldg));
}
size_t ba16_dqv_lds_bytes(int dk, int dv, int dkt, int dvt) {
  const size_t ldk = ba16_ldk(dk), ldg = ba16_ldk(dv);
  return sizeof(float) * 4 * kBaTile +
         sizeof(uint16_t) * (kBa16Rows * (ldk + ldg) + 2 * kBaTile * (ldk + ba16_ldv(dkt) + ldg + ba16_ldv(dvt)));
}

// the workgroup's own rows r0 .. r0 + 127 of a [*, width] fp32 matrix -> a rounded row image (rows past the window's
// end repeat its last row; they are never stored)
template <int DT>
__device__ __forceinline__ void ba16_stage_own(uint16_t *img, int ldi, int widthp, const float *__restrict__ src,
                                               int64_t ld, int64_t first, int64_t end, int width, bool vec) {
  const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);
  for (int rb = 0; rb < kBaMaxWaves; ++rb) {
    int64_t g = first + kBaTile * rb + srow;
    if (g >= end) g = end - 1;
    const float *row = src + g * ld;
    uint16_t *dst = img + (kBaTile * rb + srow) * ldi;
    for (int c0 = scol; c0 < widthp; c0 += 32) store4<DT>(dst + c0, ba16_load4(row, c0, width, vec));
  }
}

// grad_kqv[k, head: keys] of the rows of one (window, head) row block
template <int DT, int DKT>
__global__ __launch_bounds__(kBa16Threads) void k_attention16_dkey(
    const float *__restrict__ kqv, int64_t ld, const float *__restrict__ go, int64_t ld_go,
    const float *__restrict__ lse, const float *__restrict__ D, const int32_t *__restrict__ windows, BaShape sh,
    DropoutParams drop, int vec, int vec_go, float *__restrict__ gkqv, int64_t ld_g) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = ((sh.dk + 15) >> 4) * 16 + 8, dkp = ldk - 8, ldg = ((sh.dv + 15) >> 4) * 16 + 8, dvp = ldg - 8;
  constexpr int ldt = ba16_ldv(DKT);
  uint16_t *Ks = lds16, *Gs = Ks + kBa16Rows * ldk, *Qr = Gs + kBa16Rows * ldg, *Qt = Qr + 2 * kBaTile * ldk,
           *Vr = Qt + 2 * kBaTile * ldt;                   // Qr, Qt, Vr: two buffers each
  const int hw = 2 * sh.dk + sh.dv;
  const float *base = kqv + (int64_t)head * hw;
  const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);

  float4 qreg[DKT], vreg[4];
  auto fetch = [&](int j0) {       // the walked tile's rows -> registers
    int64_t g = (int64_t)start + j0 + srow;
    if (g >= end) g = end - 1;
    const float *row = base + g * ld;
#pragma unroll
    for (int t = 0; t < DKT; ++t) qreg[t] = ba16_load4(row + sh.dk, 32 * t + scol, sh.dk, vec);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < sh.dvt) vreg[t] = ba16_load4(row + 2 * sh.dk, 32 * t + scol, sh.dv, vec);
  };
  auto park = [&](int buf) {       // registers -> the rounded images: queries by rows and transposable, values by rows
    uint16_t *q = Qr + buf * kBaTile * ldk + srow * ldk, *qt = Qt + buf * kBaTile * ldt + srow * ldt,
             *v = Vr + buf * kBaTile * ldg + srow * ldg;
#pragma unroll
    for (int t = 0; t < DKT; ++t) {
      if (32 * t + scol < dkp) store4<DT>(q + 32 * t + scol, qreg[t]);
      store4<DT>(qt + 32 * t + scol, qreg[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < sh.dvt && 32 * t + scol < dvp) store4<DT>(v + 32 * t + scol, vreg[t]);
  };

  fetch(0);
  ba16_stage_own<DT>(Ks, ldk, dkp, base, ld, (int64_t)start + r0, end, sh.dk, vec);
  ba16_stage_own<DT>(Gs, ldg, dvp, go + (int64_t)head * sh.dv, ld_go, (int64_t)start + r0, end, sh.dv, vec_go);
  park(0);
  __syncthreads();

  const int wrow = r0 + kBaTile * wave;            // first row of the wave inside the window
  const bool live = wrow < n;                      // a wave without rows still stages and meets the barriers
  const int ksteps = dkp >> 4, vsteps = dvp >> 4;
  int64_t krow = (int64_t)start + wrow + c;
  if (krow >= end) krow = end - 1;                 // such lanes compute a row that is never stored
  const float lse_k = lse[krow * sh.heads + head], D_k = D[krow * sh.heads + head];
  const uint16_t *Kw = Ks + (kBaTile * wave + c) * ldk + 8 * h, *Gw = Gs + (kBaTile * wave + c) * ldg + 8 * h;
  const int tr_off = ba16_tr_off(lane, ldt);

  f32x16 g[DKT];
#pragma unroll
  for (int t = 0; t < DKT; ++t) zero(g[t]);

  int cur = 0;
  for (int j0 = 0; j0 < n; j0 += kBaTile) {
    const bool more = j0 + kBaTile < n;
    if (more) fetch(j0 + kBaTile);
    if (live) {
      // S^T[v, k] and dP^T[v, k] = value_v . dOut_k: lane = key row, registers = the tile's rows
      f32x16 x = ba16_nt<DT>(Qr + cur * kBaTile * ldk + c * ldk + 8 * h, Kw, ksteps);
      const f32x16 y = ba16_nt<DT>(Vr + cur * kBaTile * ldg + c * ldg + 8 * h, Gw, vsteps);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = j0 + ba_row(r, h);
        const float p = j < n ? ba_exp(x[r] * sh.scale - lse_k) : 0.0f;
        const float keep = drop.thr ? ba_keep(drop, krow * sh.heads + head, j) : 1.0f;
        x[r] = p * (keep * y[r] - D_k);                      // dS^T[v, k]
      }
      ba16_tn<DT, DKT, ldt>(g, x, Qt + cur * kBaTile * ldt + tr_off);
    }
    if (more) park(cur ^ 1);
    __syncthreads();                 // the other buffer is complete; everyone is done reading this one
    cur ^= 1;
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wrow + ba_row(r, h);
    if (row < n) {
      float *dst = gkqv + ((int64_t)start + row) * ld_g + (int64_t)head * hw;
#pragma unroll
      for (int t = 0; t < DKT; ++t)
        if (32 * t + c < sh.dk) dst[32 * t + c] = g[t][r] * sh.scale;
    }
  }
}

// grad_kqv[v, head: queries | values] of the rows of one (window, head) row block
template <int DT, int DKT, int DVT>
__global__ __launch_bounds__(kBa16Threads) void k_attention16_dqv(
    const float *__restrict__ kqv, int64_t ld, const float *__restrict__ go, int64_t ld_go,
    const float *__restrict__ lse, const float *__restrict__ D, const int32_t *__restrict__ windows, BaShape sh,
    DropoutParams drop, int vec, int vec_go, float *__restrict__ gkqv, int64_t ld_g) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds16[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = ((sh.dk + 15) >> 4) * 16 + 8, dkp = ldk - 8, ldg = ((sh.dv + 15) >> 4) * 16 + 8, dvp = ldg - 8;
  constexpr int ltk = ba16_ldv(DKT), ltv = ba16_ldv(DVT);
  float *stats = reinterpret_cast<float *>(lds16);        // two buffers of [lse of the tile's 32 rows | their D]
  uint16_t *Qs = lds16 + 8 * kBaTile, *Vs = Qs + kBa16Rows * ldk, *Kr = Vs + kBa16Rows * ldg,
           *Kt = Kr + 2 * kBaTile * ldk, *Gr = Kt + 2 * kBaTile * ltk, *Gt = Gr + 2 * kBaTile * ldg;
  const int hw = 2 * sh.dk + sh.dv;
  const float *base = kqv + (int64_t)head * hw, *gbase = go + (int64_t)head * sh.dv;
  const int srow = threadIdx.x >> 3, scol = 4 * (threadIdx.x & 7);

  float4 kreg[DKT], greg[DVT];
  float streg = 0.0f;
  auto fetch = [&](int i0) {       // the walked tile's rows -> registers
    int64_t g = (int64_t)start + i0 + srow;
    if (g >= end) g = end - 1;
#pragma unroll
    for (int t = 0; t < DKT; ++t) kreg[t] = ba16_load4(base + g * ld, 32 * t + scol, sh.dk, vec);
#pragma unroll
    for (int t = 0; t < DVT; ++t) greg[t] = ba16_load4(gbase + g * ld_go, 32 * t + scol, sh.dv, vec_go);
    if (threadIdx.x < 2 * kBaTile) {
      int64_t r = (int64_t)start + i0 + (threadIdx.x & 31);
      if (r >= end) r = end - 1;
      streg = (threadIdx.x < kBaTile ? lse : D)[r * sh.heads + head];
    }
  };
  auto park = [&](int buf) {       // registers -> the rounded images, each by rows and transposable
    uint16_t *k = Kr + buf * kBaTile * ldk + srow * ldk, *kt = Kt + buf * kBaTile * ltk + srow * ltk,
             *g = Gr + buf * kBaTile * ldg + srow * ldg, *gt = Gt + buf * kBaTile * ltv + srow * ltv;
#pragma unroll
    for (int t = 0; t < DKT; ++t) {
      if (32 * t + scol < dkp) store4<DT>(k + 32 * t + scol, kreg[t]);
      store4<DT>(kt + 32 * t + scol, kreg[t]);
    }
#pragma unroll
    for (int t = 0; t < DVT; ++t) {
      if (32 * t + scol < dvp) store4<DT>(g + 32 * t + scol, greg[t]);
      store4<DT>(gt + 32 * t + scol, greg[t]);
    }
    if (threadIdx.x < 2 * kBaTile) stats[buf * 2 * kBaTile + threadIdx.x] = streg;
  };

  fetch(0);
  ba16_stage_own<DT>(Qs, ldk, dkp, base + sh.dk, ld, (int64_t)start + r0, end, sh.dk, vec);
  ba16_stage_own<DT>(Vs, ldg, dvp, base + 2 * sh.dk, ld, (int64_t)start + r0, end, sh.dv, vec);
  park(0);
  __syncthreads();

  const int wrow = r0 + kBaTile * wave;
  const bool live = wrow < n;
  const int ksteps = dkp >> 4, vsteps = dvp >> 4;
  const int jcol = wrow + c;                       // the lane's query row = its column inside the window
  const uint16_t *Qw = Qs + (kBaTile * wave + c) * ldk + 8 * h, *Vw = Vs + (kBaTile * wave + c) * ldg + 8 * h;
  const int trk = ba16_tr_off(lane, ltk), trv = ba16_tr_off(lane, ltv);

  f32x16 gq[DKT], gv[DVT];
#pragma unroll
  for (int t = 0; t < DKT; ++t) zero(gq[t]);
#pragma unroll
  for (int t = 0; t < DVT; ++t) zero(gv[t]);

  int cur = 0;
  for (int i0 = 0; i0 < n; i0 += kBaTile) {
    const bool more = i0 + kBaTile < n;
    if (more) fetch(i0 + kBaTile);
    if (live) {
      // S[k, v] and dP[k, v] = dOut_k . value_v: lane = query row, registers = the tile's key rows
      f32x16 x = ba16_nt<DT>(Kr + cur * kBaTile * ldk + c * ldk + 8 * h, Qw, ksteps);
      f32x16 y = ba16_nt<DT>(Gr + cur * kBaTile * ldg + c * ldg + 8 * h, Vw, vsteps);
      const float *lse_t = stats + cur * 2 * kBaTile, *D_t = lse_t + kBaTile;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = ba_row(r, h), i = i0 + kk;
        const float p = i < n ? ba_exp(x[r] * sh.scale - lse_t[kk]) : 0.0f;
        const float keep = drop.thr ? ba_keep(drop, ((int64_t)start + i) * sh.heads + head, jcol) : 1.0f;
        x[r] = p * keep;                                     // (M o P)[k, v]
        y[r] = p * (keep * y[r] - D_t[kk]);                  // dS[k, v]
      }
      ba16_tn<DT, DVT, ltv>(gv, x, Gt + cur * kBaTile * ltv + trv);
      ba16_tn<DT, DKT, ltk>(gq, y, Kt + cur * kBaTile * ltk + trk);
    }
    if (more) park(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wrow + ba_row(r, h);
    if (row < n) {
      float *dst = gkqv + ((int64_t)start + row) * ld_g + (int64_t)head * hw;
#pragma unroll
      for (int t = 0; t < DKT; ++t)
        if (32 * t + c < sh.dk) dst[sh.dk + 32 * t + c] = gq[t][r] * sh.scale;
#pragma unroll
      for (int t = 0; t < DVT; ++t)
        if (32 * t + c < sh.dv) dst[2 * sh.dk + 32 * t + c] = gv[t][r];
    }
  }
}

struct Ba16BackwardArgs {
  const float *kqv;
  int64_t ld;
  const float *go;
  int64_t ld_go;
  const float *lse, *D;
  const int32_t *windows;
  BaShape sh;
  DropoutParams drop;
  int vec, vec_go;
  float *gkqv;
  int64_t ld_g;
  dim3 grid;
  hipStream_t st;
};

template <class Kern>
int ba16_launch(Kern kern, size_t bytes, const Ba16BackwardArgs &a) {
  PTGNN_REQUIRE(ba_lds_ok(kern, bytes), PTGNN_AMD_EHIP, "selfatt_train16_backward: %zu bytes of LDS refused", bytes);
  kern<<<a.grid, kBa16Threads, bytes, a.st>>>(a.kqv, a.ld, a.go, a.ld_go, a.lse, a.D, a.windows, a.sh, a.drop, a.vec,
                                              a.vec_go, a.gkqv, a.ld_g);
  return PTGNN_AMD_OK;
}

template <int DT, int DKT>
int ba16_launch_dqv(int dvt, size_t bytes, const Ba16BackwardArgs &a) {
  int rc = PTGNN_AMD_OK;
  BA_TILES(dvt, rc = ba16_launch(k_attention16_dqv<DT, DKT, TT>, bytes, a))
  return rc;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_selfatt_train16_supported(int32_t dk, int32_t dv, int32_t dtype) {
  return half16::dtype_ok(dtype) && dk >= 1 && dk <= kBaMaxDim && dv >= 1 && dv <= kBaMaxDim ? 1 : 0;
}

extern "C" int ptgnn_amd_selfatt_train16_backward(const float *kqv, int64_t ld_kqv, const float *out, int64_t ld_out,
                                                  const float *lse, const float *grad_out, int64_t ld_go,
                                                  const int32_t *windows, int64_t num_windows, int64_t num_rows,
                                                  int32_t max_num_nodes, int32_t num_heads, int32_t dk, int32_t dv,
                                                  float dropout_p, uint64_t seed, float *grad_kqv, int64_t ld_gkqv,
                                                  void *workspace, size_t workspace_bytes, int32_t dtype,
                                                  void *stream_) {
  const char *what = "selfatt_train16_backward";
  PTGNN_REQUIRE(half16::dtype_ok(dtype), PTGNN_AMD_EINVAL, "%s: unknown dtype id %d", what, dtype);
  const int rc = ba_check(what, kqv, ld_kqv, windows, num_windows, num_rows, max_num_nodes, num_heads, dk, dv, dropout_p);
  if (rc != PTGNN_AMD_OK || num_rows == 0) return rc;
  PTGNN_REQUIRE(out && lse && grad_out && grad_kqv, PTGNN_AMD_EINVAL, "%s: null pointer", what);
  PTGNN_REQUIRE(ld_out >= (int64_t)num_heads * dv && ld_go >= (int64_t)num_heads * dv &&
                    ld_gkqv >= (int64_t)num_heads * (2 * dk + dv),
                PTGNN_AMD_EINVAL, "%s: bad leading dimension", what);
  PTGNN_REQUIRE(half16::aligned4(kqv) && half16::aligned4(grad_out), PTGNN_AMD_EINVAL,
                "%s: kqv / grad_out is not 4-byte aligned", what);
  const size_t need = ((size_t)num_rows * num_heads * sizeof(float) + 255) / 256 * 256;
  PTGNN_REQUIRE(workspace && workspace_bytes >= need, PTGNN_AMD_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", what,
                workspace_bytes, need);
  const int dkt = (dk + 31) / 32, dvt = (dv + 31) / 32;
  const size_t key_bytes = ba16_dkey_lds_bytes(dk, dv, dkt), qv_bytes = ba16_dqv_lds_bytes(dk, dv, dkt, dvt);
  Ba16BackwardArgs a;
  a.sh = ba_shape(num_heads, dk, dv, kBaMaxWaves, num_rows, max_num_nodes);
  PTGNN_REQUIRE(num_windows * a.sh.row_tiles < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED, "%s: too many windows", what);
  a.kqv = kqv, a.ld = ld_kqv, a.go = grad_out, a.ld_go = ld_go, a.lse = lse, a.windows = windows;
  a.D = static_cast<float *>(workspace);
  a.drop = ba_dropout(dropout_p, seed, max_num_nodes);
  // every float4 of a head's keys, queries and values / of its dOut columns is 16-byte aligned
  a.vec = half16::rows16(kqv, ld_kqv) && dk % 4 == 0 && dv % 4 == 0 ? 1 : 0;
  a.vec_go = half16::rows16(grad_out, ld_go) && dv % 4 == 0 ? 1 : 0;
  a.gkqv = grad_kqv, a.ld_g = ld_gkqv;
  a.grid = dim3((unsigned)(num_windows * a.sh.row_tiles), (unsigned)num_heads);
  a.st = (hipStream_t)stream_;
  k_block_attention_rowdot<<<(unsigned)((num_rows * num_heads + 255) / 256), 256, 0, a.st>>>(
      grad_out, ld_go, out, ld_out, num_rows, num_heads, dv, static_cast<float *>(workspace));
  PTGNN_LAUNCH_CHECK();
  int rc2 = PTGNN_AMD_OK;
  half16::with_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    BA_TILES(dkt, rc2 = ba16_launch(k_attention16_dkey<DT, TT>, key_bytes, a))
    if (rc2 != PTGNN_AMD_OK) return;
    BA_TILES(dkt, (rc2 = ba16_launch_dqv<DT, TT>(dvt, qv_bytes, a)))
  });
  if (rc2 != PTGNN_AMD_OK) return rc2;
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_ATTENTION_TRAIN16_BACKWARD);
  return PTGNN_AMD_OK;
}
