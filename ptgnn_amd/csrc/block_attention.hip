// Block self-attention of MultiHeadSelfAttentionMessagePassing (ptgnn/neuralmodels/gnn/messagepassing/
// selfattmessagepassing.py:59-75,104-117): the nodes of a graph are cut into WINDOWS of at most max_num_nodes consecutive
// rows, and inside a window, per head,
//
//     S[k, v] = key_k . query_v / sqrt(dk)      P = softmax_v(S)      P = dropout(P)      out_k = sum_v P[k, v] value_v
//
// (the row side is the KEY and the softmax runs over the QUERIES: the reference's order, kept).  The reference runs this
// as a Python loop of einsum / softmax / einsum per window; here it is one launch, flash-style: the [n, n] scores never
// leave the registers.  kqv [N, heads (2 dk + dv)] is read in place, per head [keys dk | queries dk | values dv].
//
// Tiling.  A workgroup of NW waves owns 32 NW consecutive rows of one (window, head); wave w its rows 32 w .. 32 w + 31,
// staged once in LDS.  The other side of the window is walked in tiles of 32 rows staged through LDS.  Both products of
// every kernel are exact-fp32 MFMAs (v_mfma_f32_32x32x2_f32):
//   * "NT":  C[i, j] = sum_d A[i, d] B[j, d] of two LDS tiles stored [row][d] (lane l feeds A[l & 31][2 s + (l >> 5)] and
//            B[l & 31][2 s + (l >> 5)] to step s).  C has j on the lane and i = (r & 3) + 8 (r >> 2) + 4 (l >> 5) in
//            register r.
//   * "TN":  Z[i, j] += sum_r X[r, i] B[r, j] with X an ACCUMULATOR tile: register s of X is the A operand of step s, and
//            the B operand of that step is row (s & 3) + 8 (s >> 2) + 4 (l >> 5) of the LDS tile -- the summed index is
//            X's register index, so the probabilities go from one product into the next without touching LDS.
// So every kernel forms its score tile with the SUMMED side of the second product in the registers: the forward and the
// key-gradient kernel hold S^T[v, k] (lane = key row k: the softmax statistics of a row live in one lane pair), the
// query / value-gradient kernel holds S[k, v] (lane = query row v).  d is zero-padded to a multiple of 32 in LDS only.
//
// Forward: online softmax (running max m and sum l per row, accumulator rescaled by exp(m_old - m_new) per tile), the
// division by l at the end, lse = m + log(l) saved per (row, head).  Dropout multiplies the unnormalised probabilities
// after they were added to l, which equals the reference's dropout(softmax(S)).
// Backward: P = exp(S - lse) is recomputed, D_k = sum_d dOut[k, d] out[k, d] (a small kernel), dS = P o (M o dP - D) with
// dP[k, v] = dOut_k . value_v and M the dropout multiplier:
//     d key_k   = scale sum_v dS[k, v] query_v        workgroup owns key rows, walks the window   (k_block_attention_dkey)
//     d query_v = scale sum_k dS[k, v] key_k          workgroup owns query rows, walks the window (k_block_attention_dqv)
//     d value_v = sum_k (M o P)[k, v] dOut_k
// Every sum runs in tile order inside one wave: no atomics, deterministic, and a window's result does not depend on where
// the window sits in the batch.
//
// Dropout is the stateless hash of dense_common.h: element (global row r, head h, window column j) takes the multiplier of
// row r heads + h, column j of a [N heads, W] mask with W = max_num_nodes rounded up to even.
#include "block_attention.h"
#include "segment_chunks.h"   // SegmentScan: the window table is the chunk table's scan with another count

namespace ptgnn_amd {
namespace {

// dst[r][c] (row stride ldd) = src[min(row0 + r, row_end - 1)][c] for c < width, 0 for width <= c < widthp
__device__ __forceinline__ void ba_stage(float *__restrict__ dst, int ldd, const float *__restrict__ src, int64_t ld,
                                         int row0, int row_end, int rows, int width, int widthp) {
  const int step = blockDim.x >> 5;
  for (int r = threadIdx.x >> 5; r < rows; r += step) {
    int64_t g = (int64_t)row0 + r;
    if (g >= row_end) g = row_end - 1;
    const float *p = src + g * ld;
    for (int c = threadIdx.x & 31; c < widthp; c += 32) dst[r * ldd + c] = c < width ? p[c] : 0.0f;
  }
}

// C[i, j] = sum_d A[i, d] B[j, d]
__device__ __forceinline__ f32x16 ba_nt(const float *__restrict__ A, int lda, const float *__restrict__ B, int ldb,
                                        int ksteps, int lane) {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.0f;
  const float *a = A + (lane & 31) * lda + (lane >> 5);
  const float *b = B + (lane & 31) * ldb + (lane >> 5);
  for (int s = 0; s < ksteps; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], b[2 * s], c, 0, 0, 0);
  return c;
}

// Z_t[i, j] += sum_r X[r, i] B[r, 32 t + j], t < T
template <int T>
__device__ __forceinline__ void ba_tn(f32x16 (&z)[T], const f32x16 &x, const float *__restrict__ B, int ldb, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const float *b = B + ba_row(s, h) * ldb + (lane & 31);
#pragma unroll
    for (int t = 0; t < T; ++t) z[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s], b[32 * t], z[t], 0, 0, 0);
  }
}

__device__ __forceinline__ float ba_keep(const DropoutParams &d, int64_t row, int j) {
  const uint32_t b = dropout_bits(d, row, j >> 1);
  return ((j & 1) ? (b >> 16) : (b & 0xffffu)) >= d.thr ? d.scale : 0.0f;
}

// One workgroup builds the window table: windows[w] = first row of window w for the W windows of the batch (graph g owns
// the rows rowptr[g] .. rowptr[g + 1] - 1 and is cut every max_nodes rows), windows[W .. bound] = num_rows.
__global__ __launch_bounds__(256) void k_attention_windows(const int32_t *__restrict__ rowptr, int num_graphs,
                                                           int max_nodes, int num_rows, int bound,
                                                           int32_t *__restrict__ windows) {
  __shared__ SegmentScan<256> scan;
  scan.begin();
  for (int base = 0; base < num_graphs; base += 256) {
    const int g = base + threadIdx.x;
    const int first = g < num_graphs ? rowptr[g] : 0;
    const int cnt = g < num_graphs ? rowptr[g + 1] - first : 0;
    const int c = cnt > 0 ? (cnt - 1) / max_nodes + 1 : 0;
    const int run = scan.step(c);
    for (int q = 0; q < c; ++q)
      if (run + q <= bound) windows[run + q] = first + q * max_nodes;
  }
  for (int i = scan.total() + threadIdx.x; i <= bound; i += 256) windows[i] = num_rows;
}

// out[k, head dv + :] and lse[k, head] of the rows of one (window, head) row block
template <int DVT>
__global__ __launch_bounds__(64 * kBaMaxWaves) void k_block_attention(
    const float *__restrict__ kqv, int64_t ld, const int32_t *__restrict__ windows, BaShape sh, DropoutParams drop,
    float *__restrict__ out, int64_t ld_out, float *__restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = 32 * sh.dkt + 1, ldv = 32 * DVT + 1;
  float *Ks = lds, *Qs = Ks + kBaTile * nw * ldk, *Vs = Qs + kBaTile * ldk;
  const float *base = kqv + (int64_t)head * (2 * sh.dk + sh.dv);
  ba_stage(Ks, ldk, base, ld, start + r0, end, kBaTile * nw, sh.dk, 32 * sh.dkt);
  const float *Kw = Ks + kBaTile * wave * ldk;
  const int wrow = r0 + kBaTile * wave;            // first row of the wave inside the window
  const bool live = wrow < n;                      // a wave without rows still stages and meets the barriers
  const int ksteps = (sh.dk + 1) >> 1;
  const int64_t krow = (int64_t)start + wrow + c;  // the lane's key row (not stored when >= end)

  f32x16 o[DVT];
#pragma unroll
  for (int t = 0; t < DVT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.0f;
  float m = -INFINITY, l = 0.0f;

  for (int j0 = 0; j0 < n; j0 += kBaTile) {
    __syncthreads();
    ba_stage(Qs, ldk, base + sh.dk, ld, start + j0, end, kBaTile, sh.dk, 32 * sh.dkt);
    ba_stage(Vs, ldv, base + 2 * sh.dk, ld, start + j0, end, kBaTile, sh.dv, 32 * DVT);
    __syncthreads();
    if (!live) continue;
    f32x16 x = ba_nt(Qs, ldk, Kw, ldk, ksteps, lane);       // S^T[v, k]: lane = key row, registers = queries
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = j0 + ba_row(r, h) < n ? x[r] * sh.scale : -INFINITY;
      tmax = fmaxf(tmax, x[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mnew = fmaxf(m, tmax);                      // finite: column j0 is inside the window
    const float alpha = ba_exp(m - mnew);
    float psum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = ba_exp(x[r] - mnew);
      psum += x[r];
    }
    psum += __shfl_xor(psum, 32, 64);
    l = l * alpha + psum;
    m = mnew;
    if (drop.thr) {
#pragma unroll
      for (int r = 0; r < 16; ++r) x[r] *= ba_keep(drop, krow * sh.heads + head, j0 + ba_row(r, h));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = __shfl(alpha, ba_row(r, h), 64);      // the rescale of accumulator row r lives in that row's lane
#pragma unroll
      for (int t = 0; t < DVT; ++t) o[t][r] *= a;
    }
    ba_tn<DVT>(o, x, Vs, ldv, lane);
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

// D[r, head] = sum_d grad_out[r, head dv + d] out[r, head dv + d], d ascending
__global__ __launch_bounds__(256) void k_block_attention_rowdot(const float *__restrict__ go, int64_t ld_go,
                                                                const float *__restrict__ out, int64_t ld_out,
                                                                int64_t num_rows, int heads, int dv,
                                                                float *__restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_rows * heads) return;
  const int64_t r = i / heads;
  const int head = (int)(i % heads);
  const float *a = go + r * ld_go + (int64_t)head * dv, *b = out + r * ld_out + (int64_t)head * dv;
  float t = 0.0f;
  for (int d = 0; d < dv; ++d) t = fmaf(a[d], b[d], t);
  D[i] = t;
}

// grad_kqv[k, head: keys] of the rows of one (window, head) row block
template <int DKT>
__global__ __launch_bounds__(64 * kBaMaxWaves) void k_block_attention_dkey(
    const float *__restrict__ kqv, int64_t ld, const float *__restrict__ go, int64_t ld_go,
    const float *__restrict__ lse, const float *__restrict__ D, const int32_t *__restrict__ windows, BaShape sh,
    DropoutParams drop, float *__restrict__ gkqv, int64_t ld_g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = 32 * DKT + 1, ldv = 32 * sh.dvt + 1;
  float *Ks = lds, *Gs = Ks + kBaTile * nw * ldk, *Qs = Gs + kBaTile * nw * ldv, *Vs = Qs + kBaTile * ldk;
  const int hw = 2 * sh.dk + sh.dv;
  const float *base = kqv + (int64_t)head * hw;
  ba_stage(Ks, ldk, base, ld, start + r0, end, kBaTile * nw, sh.dk, 32 * DKT);
  ba_stage(Gs, ldv, go + (int64_t)head * sh.dv, ld_go, start + r0, end, kBaTile * nw, sh.dv, 32 * sh.dvt);
  const float *Kw = Ks + kBaTile * wave * ldk, *Gw = Gs + kBaTile * wave * ldv;
  const int wrow = r0 + kBaTile * wave;
  const bool live = wrow < n;
  const int ksteps = (sh.dk + 1) >> 1, vsteps = (sh.dv + 1) >> 1;
  int64_t krow = (int64_t)start + wrow + c;
  if (krow >= end) krow = end - 1;                 // such lanes compute a row that is never stored
  const float lse_k = lse[krow * sh.heads + head], D_k = D[krow * sh.heads + head];

  f32x16 g[DKT];
#pragma unroll
  for (int t = 0; t < DKT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[t][r] = 0.0f;

  for (int j0 = 0; j0 < n; j0 += kBaTile) {
    __syncthreads();
    ba_stage(Qs, ldk, base + sh.dk, ld, start + j0, end, kBaTile, sh.dk, 32 * DKT);
    ba_stage(Vs, ldv, base + 2 * sh.dk, ld, start + j0, end, kBaTile, sh.dv, 32 * sh.dvt);
    __syncthreads();
    if (!live) continue;
    f32x16 x = ba_nt(Qs, ldk, Kw, ldk, ksteps, lane);       // S^T[v, k]
    const f32x16 y = ba_nt(Vs, ldv, Gw, ldv, vsteps, lane); // dP^T[v, k] = value_v . dOut_k
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + ba_row(r, h);
      const float p = j < n ? ba_exp(x[r] * sh.scale - lse_k) : 0.0f;
      const float keep = drop.thr ? ba_keep(drop, krow * sh.heads + head, j) : 1.0f;
      x[r] = p * (keep * y[r] - D_k);                       // dS^T[v, k]
    }
    ba_tn<DKT>(g, x, Qs, ldk, lane);
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
template <int DKT, int DVT>
__global__ __launch_bounds__(64 * kBaMaxWaves) void k_block_attention_dqv(
    const float *__restrict__ kqv, int64_t ld, const float *__restrict__ go, int64_t ld_go,
    const float *__restrict__ lse, const float *__restrict__ D, const int32_t *__restrict__ windows, BaShape sh,
    DropoutParams drop, float *__restrict__ gkqv, int64_t ld_g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int start, end, r0;
  if (!ba_locate(windows, sh, start, end, r0)) return;
  const int n = end - start;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  const int head = blockIdx.y;
  const int ldk = 32 * DKT + 1, ldv = 32 * DVT + 1;
  float *Qs = lds, *Vs = Qs + kBaTile * nw * ldk, *Ks = Vs + kBaTile * nw * ldv, *Gs = Ks + kBaTile * ldk;
  float *lse_t = Gs + kBaTile * ldv, *D_t = lse_t + kBaTile;
  const int hw = 2 * sh.dk + sh.dv;
  const float *base = kqv + (int64_t)head * hw;
  ba_stage(Qs, ldk, base + sh.dk, ld, start + r0, end, kBaTile * nw, sh.dk, 32 * DKT);
  ba_stage(Vs, ldv, base + 2 * sh.dk, ld, start + r0, end, kBaTile * nw, sh.dv, 32 * DVT);
  const float *Qw = Qs + kBaTile * wave * ldk, *Vw = Vs + kBaTile * wave * ldv;
  const int wrow = r0 + kBaTile * wave;
  const bool live = wrow < n;
  const int ksteps = (sh.dk + 1) >> 1, vsteps = (sh.dv + 1) >> 1;
  const int jcol = wrow + c;                       // the lane's query row = its column inside the window

  f32x16 gq[DKT], gv[DVT];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int t = 0; t < DKT; ++t) gq[t][r] = 0.0f;
#pragma unroll
    for (int t = 0; t < DVT; ++t) gv[t][r] = 0.0f;
  }

  for (int i0 = 0; i0 < n; i0 += kBaTile) {
    __syncthreads();
    ba_stage(Ks, ldk, base, ld, start + i0, end, kBaTile, sh.dk, 32 * DKT);
    ba_stage(Gs, ldv, go + (int64_t)head * sh.dv, ld_go, start + i0, end, kBaTile, sh.dv, 32 * DVT);
    if (threadIdx.x < kBaTile) {
      int64_t r = (int64_t)start + i0 + threadIdx.x;
      if (r >= end) r = end - 1;
      lse_t[threadIdx.x] = lse[r * sh.heads + head];
      D_t[threadIdx.x] = D[r * sh.heads + head];
    }
    __syncthreads();
    if (!live) continue;
    f32x16 x = ba_nt(Ks, ldk, Qw, ldk, ksteps, lane);       // S[k, v]: lane = query row, registers = keys
    f32x16 y = ba_nt(Gs, ldv, Vw, ldv, vsteps, lane);       // dP[k, v] = dOut_k . value_v
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = ba_row(r, h), i = i0 + kk;
      const float p = i < n ? ba_exp(x[r] * sh.scale - lse_t[kk]) : 0.0f;
      const float keep = drop.thr ? ba_keep(drop, ((int64_t)start + i) * sh.heads + head, jcol) : 1.0f;
      x[r] = p * keep;                                      // (M o P)[k, v]
      y[r] = p * (keep * y[r] - D_t[kk]);                   // dS[k, v]
    }
    ba_tn<DVT>(gv, x, Gs, ldv, lane);
    ba_tn<DKT>(gq, y, Ks, ldk, lane);
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

// LDS floats of a workgroup of nw waves: `own` row images of 32 nw rows and one 32-row tile of each of `walk`
size_t ba_lds_bytes(int nw, int own_ld, int walk_ld, int extra) {
  return sizeof(float) * ((size_t)kBaTile * nw * own_ld + (size_t)kBaTile * walk_ld + extra);
}

// the most waves (4, 2, 1) whose LDS stays within 64 KiB; one wave when none does (at most 67 KiB then)
int ba_waves(int own_ld, int walk_ld, int extra) {
  for (int nw = kBaMaxWaves; nw > 1; nw >>= 1)
    if (ba_lds_bytes(nw, own_ld, walk_ld, extra) <= 64 * 1024) return nw;
  return 1;
}

int64_t ba_windows_bound(int64_t num_graphs, int64_t num_rows, int64_t max_nodes) {
  return (num_rows + max_nodes - 1) / max_nodes + num_graphs;
}

DropoutParams ba_dropout(float p, uint64_t seed, int32_t max_nodes) {
  return make_dropout(p, seed, (max_nodes + 1) / 2 * 2);
}

template <int DKT>
int ba_launch_dqv(int dvt, dim3 grid, int nw, size_t bytes, hipStream_t st, const float *kqv, int64_t ld, const float *go,
                  int64_t ld_go, const float *lse, const float *D, const int32_t *windows, const BaShape &sh,
                  const DropoutParams &drop, float *gkqv, int64_t ld_g) {
  BA_TILES(dvt, {
    auto kern = k_block_attention_dqv<DKT, TT>;
    PTGNN_REQUIRE(ba_lds_ok(kern, bytes), PTGNN_AMD_EHIP, "block_attention_backward: %zu bytes of LDS refused", bytes);
    kern<<<grid, 64 * nw, bytes, st>>>(kqv, ld, go, ld_go, lse, D, windows, sh, drop, gkqv, ld_g);
  })
  return PTGNN_AMD_OK;
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_block_attention_supported(int32_t dk, int32_t dv) {
  return dk >= 1 && dk <= kBaMaxDim && dv >= 1 && dv <= kBaMaxDim ? 1 : 0;
}

extern "C" int64_t ptgnn_amd_attention_windows_bound(int64_t num_graphs, int64_t num_rows, int32_t max_num_nodes) {
  if (num_graphs < 0 || num_rows < 0 || max_num_nodes <= 0) return -1;
  return ba_windows_bound(num_graphs, num_rows, max_num_nodes);
}

extern "C" int ptgnn_amd_attention_windows(const int32_t *rowptr, int64_t num_graphs, int64_t num_rows,
                                           int32_t max_num_nodes, int32_t *windows, int64_t capacity, void *stream_) {
  PTGNN_REQUIRE(num_graphs >= 0 && num_rows >= 0 && max_num_nodes > 0, PTGNN_AMD_EINVAL,
                "attention_windows (block_attention): bad sizes");
  PTGNN_REQUIRE(num_graphs > 0 || num_rows == 0, PTGNN_AMD_EINVAL,
                "attention_windows (block_attention): rows without graphs");
  PTGNN_REQUIRE(rowptr && windows, PTGNN_AMD_EINVAL, "attention_windows (block_attention): null pointer");
  const int64_t bound = ba_windows_bound(num_graphs, num_rows, max_num_nodes);
  PTGNN_REQUIRE(bound < ((int64_t)1 << 31) - 1 && num_rows < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "attention_windows (block_attention): too many graphs / rows");
  PTGNN_REQUIRE(capacity >= bound + 1, PTGNN_AMD_EINVAL,
                "attention_windows (block_attention): table of %lld entries, need %lld", (long long)capacity,
                (long long)(bound + 1));
  k_attention_windows<<<1, 256, 0, (hipStream_t)stream_>>>(rowptr, (int)num_graphs, max_num_nodes, (int)num_rows,
                                                           (int)bound, windows);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_block_attention_f32(const float *kqv, int64_t ld_kqv, const int32_t *windows,
                                             int64_t num_windows, int64_t num_rows, int32_t max_num_nodes,
                                             int32_t num_heads, int32_t dk, int32_t dv, float dropout_p, uint64_t seed,
                                             float *out, int64_t ld_out, float *lse, void *stream_) {
  const int rc = ba_check("block_attention", kqv, ld_kqv, windows, num_windows, num_rows, max_num_nodes, num_heads, dk,
                          dv, dropout_p);
  if (rc != PTGNN_AMD_OK || num_rows == 0) return rc;
  PTGNN_REQUIRE(out && lse, PTGNN_AMD_EINVAL, "block_attention: null pointer");
  PTGNN_REQUIRE(ld_out >= (int64_t)num_heads * dv, PTGNN_AMD_EINVAL, "block_attention: bad leading dimension");
  const int dkt = (dk + 31) / 32, dvt = (dv + 31) / 32;
  const int ldk = 32 * dkt + 1, ldv = 32 * dvt + 1;
  // own: keys; walked: queries + values
  const int nw = ba_waves(ldk, ldk + ldv, 0);
  const size_t bytes = ba_lds_bytes(nw, ldk, ldk + ldv, 0);
  const BaShape sh = ba_shape(num_heads, dk, dv, nw, num_rows, max_num_nodes);
  PTGNN_REQUIRE(num_windows * sh.row_tiles < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "block_attention: too many windows");
  const DropoutParams drop = ba_dropout(dropout_p, seed, max_num_nodes);
  const dim3 grid((unsigned)(num_windows * sh.row_tiles), (unsigned)num_heads);
  hipStream_t st = (hipStream_t)stream_;
  BA_TILES(dvt, {
    auto kern = k_block_attention<TT>;
    PTGNN_REQUIRE(ba_lds_ok(kern, bytes), PTGNN_AMD_EHIP, "block_attention: %zu bytes of LDS refused", bytes);
    kern<<<grid, 64 * nw, bytes, st>>>(kqv, ld_kqv, windows, sh, drop, out, ld_out, lse);
  })
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BLOCK_ATTENTION);
  return PTGNN_AMD_OK;
}

extern "C" size_t ptgnn_amd_block_attention_backward_workspace_bytes(int64_t num_rows, int32_t num_heads) {
  if (num_rows <= 0 || num_heads <= 0) return 0;
  return ((size_t)num_rows * num_heads * sizeof(float) + 255) / 256 * 256;
}

extern "C" int ptgnn_amd_block_attention_backward_f32(const float *kqv, int64_t ld_kqv, const float *out, int64_t ld_out,
                                                      const float *lse, const float *grad_out, int64_t ld_go,
                                                      const int32_t *windows, int64_t num_windows, int64_t num_rows,
                                                      int32_t max_num_nodes, int32_t num_heads, int32_t dk, int32_t dv,
                                                      float dropout_p, uint64_t seed, float *grad_kqv, int64_t ld_gkqv,
                                                      void *workspace, size_t workspace_bytes, void *stream_) {
  const int rc = ba_check("block_attention_backward", kqv, ld_kqv, windows, num_windows, num_rows, max_num_nodes,
                          num_heads, dk, dv, dropout_p);
  if (rc != PTGNN_AMD_OK || num_rows == 0) return rc;
  PTGNN_REQUIRE(out && lse && grad_out && grad_kqv, PTGNN_AMD_EINVAL, "block_attention_backward: null pointer");
  PTGNN_REQUIRE(ld_out >= (int64_t)num_heads * dv && ld_go >= (int64_t)num_heads * dv &&
                    ld_gkqv >= (int64_t)num_heads * (2 * dk + dv),
                PTGNN_AMD_EINVAL, "block_attention_backward: bad leading dimension");
  const size_t need = ptgnn_amd_block_attention_backward_workspace_bytes(num_rows, num_heads);
  PTGNN_REQUIRE(workspace && workspace_bytes >= need, PTGNN_AMD_EWORKSPACE,
                "block_attention_backward: workspace of %zu bytes, need %zu", workspace_bytes, need);
  const int dkt = (dk + 31) / 32, dvt = (dv + 31) / 32;
  const int ldk = 32 * dkt + 1, ldv = 32 * dvt + 1;
  // both kernels: own two row images (keys + dOut, or queries + values), walk two tiles (+ lse and D of a tile)
  const int nw = ba_waves(ldk + ldv, ldk + ldv, 2 * kBaTile);
  const size_t bytes = ba_lds_bytes(nw, ldk + ldv, ldk + ldv, 2 * kBaTile);
  const BaShape sh = ba_shape(num_heads, dk, dv, nw, num_rows, max_num_nodes);
  PTGNN_REQUIRE(num_windows * sh.row_tiles < ((int64_t)1 << 31), PTGNN_AMD_EUNSUPPORTED,
                "block_attention_backward: too many windows");
  const DropoutParams drop = ba_dropout(dropout_p, seed, max_num_nodes);
  const dim3 grid((unsigned)(num_windows * sh.row_tiles), (unsigned)num_heads);
  hipStream_t st = (hipStream_t)stream_;
  float *D = static_cast<float *>(workspace);
  k_block_attention_rowdot<<<(unsigned)((num_rows * num_heads + 255) / 256), 256, 0, st>>>(
      grad_out, ld_go, out, ld_out, num_rows, num_heads, dv, D);
  PTGNN_LAUNCH_CHECK();
  BA_TILES(dkt, {
    auto kern = k_block_attention_dkey<TT>;
    PTGNN_REQUIRE(ba_lds_ok(kern, bytes), PTGNN_AMD_EHIP, "block_attention_backward: %zu bytes of LDS refused", bytes);
    kern<<<grid, 64 * nw, bytes, st>>>(kqv, ld_kqv, grad_out, ld_go, lse, D, windows, sh, drop, grad_kqv, ld_gkqv);
  })
  PTGNN_LAUNCH_CHECK();
  int rc2 = PTGNN_AMD_OK;
  BA_TILES(dkt, rc2 = ba_launch_dqv<TT>(dvt, grid, nw, bytes, st, kqv, ld_kqv, grad_out, ld_go, lse, D, windows, sh, drop,
                                        grad_kqv, ld_gkqv))
  if (rc2 != PTGNN_AMD_OK) return rc2;
  PTGNN_LAUNCH_CHECK();
  count_launch(PTGNN_AMD_KERNEL_BLOCK_ATTENTION_BACKWARD);
  return PTGNN_AMD_OK;
}
