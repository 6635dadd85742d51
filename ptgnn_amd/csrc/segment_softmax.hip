// Segment softmax, log-softmax and logsumexp of a general [E, D] source over an arbitrary (unsorted) index, and their
// backwards: torch_scatter.composite's scatter_softmax / scatter_log_softmax / scatter_logsumexp as the facade documents
// them (ptgnn_amd/scatter.py), in two passes over the source instead of a chain of ten launches:
//     state pass   per (segment, column): m = max_seg x,  lognorm = log(sum_seg exp(x - m) + eps)      reads x once
//     write pass   y = x - m[idx] - lognorm[idx]  (log-softmax),  exp of that (softmax)               reads x, writes y
// logsumexp is the state itself: lognorm + m, -inf for a segment without elements.
//
// ONE WALK, THREE FOLDS.  The state pass is a walk over the plan of the index (rowptr, perm: the element of every slot)
// templated on what it folds: MaxSum(x) for the forward (softmax_state.h: logits spanning more than 100 do not overflow),
// Sum(g) for the log-softmax backward, Dot(g, y) for the softmax backward.  With S the folded per-segment value:
//     log-softmax  dx = g - exp(y) S        softmax  dx = y (g - S)        logsumexp  dx = x == -inf ? 0 : g[idx] exp(x - L[idx])
// so a backward is the walk plus one element-parallel write (logsumexp: the write alone).
//
// The walk serves two regimes, split by kChunkRows (128) slots:
//   short segments (<= 128 slots)  k_short: one LANE GROUP per segment, no workspace.  A group is CT column lanes x SL
//     slot lanes; CT = D rounded up to a power of two, at most 64 (wider rows loop over column tiles), SL = min(64 / CT, 8),
//     so a wave holds 64 / (CT SL) segments: D = 1 gives 8 segments of 8 slot lanes per wave.  A slot lane takes slots
//     sl, sl + SL, ... four at a time -- four perm entries, then the four row loads, then the pushes -- and the slot lanes
//     are merged by the xor butterfly over `combine`, outside the (divergent) slot loop.
//   long segments (> 128 slots)    cut into 128-slot chunks counted from the segment's own start (segment_chunks.h).
//     The chunk table (k_long_chunk_starts, one SegmentScan launch) counts ONLY the long segments, so the grid bound is
//     2 E / 128 + 1.  k_long: one workgroup per chunk (x column tile); the chunk's perm entries are staged in LDS once;
//     threads are THREADS / CT slot lanes x CT column lanes; slot lanes merge by the butterfly inside the wave, then the
//     waves in wave order through LDS; the chunk's partial goes to the workspace.  k_fold combines the partials of a
//     segment in chunk order.
// No float atomics, and SL depends on D alone: a segment's value is a fixed function of its elements and their slot
// order, wherever it sits in the batch; the same call twice returns the same bits.
//
// The write pass (k_write) is element-parallel and coalesced in element order, reads the segment of an element from the
// index as the facade receives it (int64), uses float4 where D % 4 == 0 and everything is 16-byte aligned, and runs a
// capped grid with a grid-stride loop.  An index outside [0, n) writes NaN and reads nothing.
//
// Edges.  eps is added to the sum taken relative to the segment's true maximum.  A -inf element next to a finite one:
// -inf (log-softmax), 0 (softmax), no contribution (logsumexp), gradient g / 0 / 0.  A segment whose elements are all -inf
// keeps the state (-inf, 0): log-softmax and softmax answer NaN (x - m = -inf + inf) and logsumexp -inf, as the composed
// route does.
//
// Limits: E, n and n D below 2^31 (ptgnn_amd_segment_softmax_supported), else EUNSUPPORTED.
#include <math.h>

#include "segment_chunks.h"
#include "softmax_state.h"

namespace ptgnn_amd {
namespace {

constexpr int kShortThreads = 256;
constexpr int kMaxSlotLanes = 8;        // slot lanes of a short segment's lane group
constexpr int kWriteThreads = 256;
constexpr int kWriteMaxBlocks = 2048;   // 8 workgroups per CU; the rest is the grid-stride loop
constexpr int kMaxTileGrid = 1024;      // gridDim.y of k_long; more column tiles than that are looped over

// ---- the three folds: T the running value, pad() the value of a slot that does not exist ------------------------------
struct FoldMaxSum {
  using T = MaxSum;
  static constexpr bool kTwo = false;
  static __device__ __forceinline__ T empty() { return MaxSum{-INFINITY, 0.0f}; }
  static __device__ __forceinline__ float pad() { return -INFINITY; }
  static __device__ __forceinline__ float value(float a, float) { return a; }
  static __device__ __forceinline__ void push_four(T &t, const float (&v)[4]) { push4(t, v); }
  static __device__ __forceinline__ T merge(const T &a, const T &b) { return combine(a, b); }
};

struct FoldSum {
  using T = float;
  static constexpr bool kTwo = false;
  static __device__ __forceinline__ T empty() { return 0.0f; }
  static __device__ __forceinline__ float pad() { return 0.0f; }
  static __device__ __forceinline__ float value(float a, float) { return a; }
  static __device__ __forceinline__ void push_four(T &t, const float (&v)[4]) { t += (v[0] + v[1]) + (v[2] + v[3]); }
  static __device__ __forceinline__ T merge(const T &a, const T &b) { return a + b; }
};

struct FoldDot : FoldSum {
  static constexpr bool kTwo = true;
  static __device__ __forceinline__ float value(float a, float b) { return a * b; }
};

// element e, column c of the operand(s) of a fold
template <typename F>
__device__ __forceinline__ float fold_load(const float *__restrict__ a, int64_t ld_a, const float *__restrict__ b,
                                           int64_t ld_b, int e, int c) {
  const float av = a[(int64_t)e * ld_a + c];
  if constexpr (F::kTwo) return F::value(av, b[(int64_t)e * ld_b + c]);
  else return F::value(av, 0.0f);
}

// what a segment's folded value leaves at (segment, column) `at`: MaxSum -> p0 = m, p1 = log(s + eps) and, where asked
// for, lse = p1 + m (-inf while m is -inf: empty or all -inf); Sum / Dot -> p0 = the sum
template <typename F>
__device__ __forceinline__ void fold_finish(const typename F::T &t, int64_t at, float eps, float *__restrict__ p0,
                                            float *__restrict__ p1, float *__restrict__ lse) {
  if constexpr (std::is_same_v<typename F::T, MaxSum>) {
    const float ln = logf(t.s + eps);
    p0[at] = t.m;
    p1[at] = ln;
    if (lse) lse[at] = t.m == -INFINITY ? -INFINITY : ln + t.m;
  } else {
    p0[at] = t;
  }
}

// chunk_start[g] = chunks of the LONG segments in front of g (chunk_start[n] = all of them); one workgroup.  A thread
// takes kScanItems consecutive segments per step (10^5 segments: 13 steps of three barriers, not 98).
constexpr int kScanItems = 8;

__global__ __launch_bounds__(1024) void k_long_chunk_starts(const int32_t *__restrict__ rowptr, int num_segments,
                                                           int32_t *__restrict__ chunk_start) {
  __shared__ SegmentScan<1024> scan;
  scan.begin();
  for (int64_t base = 0; base < num_segments; base += 1024 * kScanItems) {
    const int64_t g0 = base + (int64_t)threadIdx.x * kScanItems;
    int r[kScanItems + 1], c[kScanItems], sum = 0;
#pragma unroll
    for (int k = 0; k <= kScanItems; ++k)              // unconditional loads, all in flight: past the end rowptr[n]
      r[k] = rowptr[g0 + k < num_segments ? g0 + k : num_segments];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      const int len = r[k + 1] - r[k];                 // 0 past the last segment
      c[k] = len > kChunkRows ? (len + kChunkRows - 1) / kChunkRows : 0;
      sum += c[k];
    }
    int run = scan.step(sum);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
      if (g0 + k < num_segments) {
        chunk_start[g0 + k] = run;
        run += c[k];
      }
  }
  if (threadIdx.x == 0) chunk_start[num_segments] = scan.total();
}

// Short segments: lane = segment of the wave x slot lane x column lane.  Segments longer than kChunkRows are left to
// k_long / k_fold; every other segment (the empty ones too) gets its state here.
template <typename F, int CT>
__global__ __launch_bounds__(kShortThreads) void k_short(const float *__restrict__ a, int64_t ld_a,
                                                         const float *__restrict__ b, int64_t ld_b,
                                                         const int32_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ perm, int num_segments, int dim,
                                                         float eps, float *__restrict__ p0, float *__restrict__ p1,
                                                         float *__restrict__ lse) {
  constexpr int SL = kWave / CT < kMaxSlotLanes ? kWave / CT : kMaxSlotLanes;
  constexpr int GROUP = CT * SL;
  constexpr int PER_BLOCK = kShortThreads / GROUP;
  using T = typename F::T;
  const int64_t seg64 = (int64_t)blockIdx.x * PER_BLOCK + threadIdx.x / GROUP;
  const int in_group = threadIdx.x % GROUP;
  const int cl = in_group % CT, sl = in_group / CT;
  const bool have = seg64 < num_segments;
  const int seg = have ? (int)seg64 : 0;
  int lo = 0, hi = 0;
  if (have) {
    lo = rowptr[seg];
    hi = rowptr[seg + 1];
  }
  const bool mine = have && hi - lo <= kChunkRows;
  if (!mine) hi = lo;                                  // a long (or missing) segment: no slots, no store
  for (int c0 = 0; c0 < dim; c0 += CT) {               // uniform over the wave
    const int col = c0 + cl;
    const bool ok = col < dim;
    T t = F::empty();
    for (int j0 = lo + sl; j0 < hi; j0 += 4 * SL) {
      int e[4];
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) e[u] = j0 + u * SL < hi ? perm[j0 + u * SL] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ok && e[u] >= 0 ? fold_load<F>(a, ld_a, b, ld_b, e[u], col) : F::pad();
      F::push_four(t, v);
    }
    // every lane of the wave is here: the butterfly over the group's slot lanes
#pragma unroll
    for (int o = GROUP / 2; o >= CT; o >>= 1) t = F::merge(t, lane_xor(t, o));
    if (mine && ok && sl == 0) fold_finish<F>(t, (int64_t)seg * dim + col, eps, p0, p1, lse);
  }
}

// Long segments: workgroup (b, tile) folds chunk b over the columns of its tile(s) into partial[b, dim].
template <typename F, int CT>
__global__ __launch_bounds__(CT == 1 ? 128 : 256) void k_long(const float *__restrict__ a, int64_t ld_a,
                                                              const float *__restrict__ b, int64_t ld_b,
                                                              const int32_t *__restrict__ rowptr,
                                                              const int32_t *__restrict__ perm, int num_segments,
                                                              int dim, const int32_t *__restrict__ chunk_start,
                                                              typename F::T *__restrict__ partial) {
  constexpr int THREADS = CT == 1 ? 128 : 256;         // at D = 1 a chunk has 128 values
  constexpr int SLOTS = THREADS / CT;                  // slot lanes of the workgroup
  constexpr int WAVES = THREADS / kWave;
  using T = typename F::T;
  __shared__ int32_t sperm[kChunkRows];
  __shared__ T swave[WAVES * CT];
  ChunkSpan ch;
  if (!chunk_locate(rowptr, chunk_start, num_segments, blockIdx.x, ch)) return;
  const int rows = ch.hi - ch.lo;
  const int t = threadIdx.x;
  if (t < rows) sperm[t] = perm[ch.lo + t];            // rows <= kChunkRows <= THREADS
  __syncthreads();
  const int cl = t % CT, sl = t / CT;
  const int lane = t & (kWave - 1), wave = t >> 6;
  const int tiles = (dim + CT - 1) / CT;
  for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int col = tile * CT + cl;
    const bool ok = col < dim;
    T acc = F::empty();
    for (int j0 = sl; j0 < rows; j0 += 4 * SLOTS) {
      int e[4];
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) e[u] = j0 + u * SLOTS < rows ? sperm[j0 + u * SLOTS] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ok && e[u] >= 0 ? fold_load<F>(a, ld_a, b, ld_b, e[u], col) : F::pad();
      F::push_four(acc, v);
    }
#pragma unroll
    for (int o = kWave / 2; o >= CT; o >>= 1) acc = F::merge(acc, lane_xor(acc, o));
    if (lane < CT) swave[wave * CT + lane] = acc;      // CT == 64: every lane is a column of its wave
    __syncthreads();
    if (t < CT && ok) {
      T r = swave[t];
      for (int w = 1; w < WAVES; ++w) r = F::merge(r, swave[w * CT + t]);
      partial[(int64_t)blockIdx.x * dim + col] = r;
    }
    __syncthreads();                                   // swave is written again by the next tile
  }
}

// the partials of a long segment combined in chunk order; short segments (no chunks) are k_short's
template <typename F>
__global__ __launch_bounds__(256) void k_fold(const typename F::T *__restrict__ partial,
                                              const int32_t *__restrict__ chunk_start, int dim, int64_t total, float eps,
                                              float *__restrict__ p0, float *__restrict__ p1, float *__restrict__ lse) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t g = i / dim;
  const int c = (int)(i - g * dim);
  const int c0 = chunk_start[g], c1 = chunk_start[g + 1];
  if (c0 == c1) return;
  typename F::T r = partial[(int64_t)c0 * dim + c];
  int k = c0 + 1;
  for (; k + 4 <= c1; k += 4) {                        // four loads in flight, one chain of merges
    const typename F::T a0 = partial[(int64_t)k * dim + c], a1 = partial[(int64_t)(k + 1) * dim + c],
                        a2 = partial[(int64_t)(k + 2) * dim + c], a3 = partial[(int64_t)(k + 3) * dim + c];
    r = F::merge(F::merge(F::merge(F::merge(r, a0), a1), a2), a3);
  }
  for (; k < c1; ++k) r = F::merge(r, partial[(int64_t)k * dim + c]);
  fold_finish<F>(r, i, eps, p0, p1, lse);
}

// ---- the write pass --------------------------------------------------------------------------------------------------
// a, b: element rows; u, w: the per-segment values p0, p1 of the element's segment
template <int MODE>
__device__ __forceinline__ float write_value(float a, float b, float u, float w) {
  if constexpr (MODE == PTGNN_AMD_SSM_LOG_SOFTMAX) return a - u - w;
  else if constexpr (MODE == PTGNN_AMD_SSM_SOFTMAX) return expf(a - u - w);
  else if constexpr (MODE == PTGNN_AMD_SSM_LOG_SOFTMAX_BACKWARD) return a - expf(b) * u;    // a = g, b = y, u = sum g
  else if constexpr (MODE == PTGNN_AMD_SSM_SOFTMAX_BACKWARD) return b * (a - u);           // a = g, b = y, u = sum g y
  else return a == -INFINITY ? 0.0f : u * expf(a - w);                                       // a = x, u = g, w = L
}

template <int MODE, int VEC>
__global__ __launch_bounds__(kWriteThreads) void k_write(const float *__restrict__ a, int64_t ld_a,
                                                         const float *__restrict__ b, int64_t ld_b,
                                                         const int64_t *__restrict__ index, const float *__restrict__ p0,
                                                         const float *__restrict__ p1, int64_t num_segments,
                                                         int64_t num_elements, int dim, float *__restrict__ out,
                                                         int64_t ld_out) {
  constexpr bool kUsesB = MODE == PTGNN_AMD_SSM_LOG_SOFTMAX_BACKWARD || MODE == PTGNN_AMD_SSM_SOFTMAX_BACKWARD;
  constexpr bool kUsesP1 = MODE == PTGNN_AMD_SSM_LOG_SOFTMAX || MODE == PTGNN_AMD_SSM_SOFTMAX ||
                           MODE == PTGNN_AMD_SSM_LOGSUMEXP_BACKWARD;
  const int per_row = dim / VEC;
  const int64_t total = num_elements * per_row;
  const int64_t step = (int64_t)gridDim.x * kWriteThreads;
  for (int64_t i = (int64_t)blockIdx.x * kWriteThreads + threadIdx.x; i < total; i += step) {
    const int64_t e = i / per_row;
    const int c = (int)(i - e * per_row) * VEC;
    const int64_t seg = index[e];
    float o[VEC];
    if (seg < 0 || seg >= num_segments) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = NAN;
    } else {
      float av[VEC], bv[VEC], uv[VEC], wv[VEC];
      vec_load<VEC>(a + e * ld_a + c, av);
      vec_load<VEC>(p0 + seg * dim + c, uv);
      if constexpr (kUsesB) vec_load<VEC>(b + e * ld_b + c, bv);
      if constexpr (kUsesP1) vec_load<VEC>(p1 + seg * dim + c, wv);
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        o[k] = write_value<MODE>(av[k], kUsesB ? bv[k] : 0.0f, uv[k], kUsesP1 ? wv[k] : 0.0f);
    }
    vec_store<VEC>(out + e * ld_out + c, o);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
// upper bound of the chunks of the long segments: a segment of len > 128 has ceil(len / 128) < 2 len / 128 of them
int64_t long_chunk_bound(int64_t elements) { return 2 * elements / kChunkRows + 1; }

bool softmax_supported(int64_t segments, int64_t elements, int64_t dim) {
  const int64_t lim = (int64_t)1 << 31;
  return segments >= 0 && elements >= 0 && dim >= 1 && segments < lim && elements < lim && dim < lim &&
         (segments == 0 || dim <= (lim - 1) / segments);
}

// the chunk table of the long segments and their chunks' partial values [bound, dim]
struct SoftmaxWorkspace {
  size_t chunk_start, partial, total;
};

SoftmaxWorkspace softmax_workspace(int64_t segments, int64_t elements, int dim, int fold) {
  const size_t value = fold == PTGNN_AMD_SSM_FOLD_MAXSUM ? sizeof(MaxSum) : sizeof(float);
  Carve c;
  SoftmaxWorkspace w;
  w.chunk_start = c.take(chunk_table_bytes(segments));
  w.partial = c.take((size_t)long_chunk_bound(elements) * (size_t)dim * value);
  w.total = c.off;
  return w;
}

int column_lanes(int dim) {
  int ct = 1;
  while (ct < dim && ct < kWave) ct <<= 1;
  return ct;
}

template <typename F, int CT>
void launch_walk(const float *a, int64_t ld_a, const float *b, int64_t ld_b, const int32_t *rowptr, const int32_t *perm,
                 int num_segments, int64_t num_elements, int dim, float eps, float *p0, float *p1, float *lse,
                 const int32_t *chunk_start, void *partial_, hipStream_t st) {
  using T = typename F::T;
  T *partial = static_cast<T *>(partial_);
  constexpr int SL = kWave / CT < kMaxSlotLanes ? kWave / CT : kMaxSlotLanes;
  constexpr int PER_BLOCK = kShortThreads / (CT * SL);
  const unsigned short_blocks = (unsigned)(((int64_t)num_segments + PER_BLOCK - 1) / PER_BLOCK);
  k_short<F, CT><<<short_blocks, kShortThreads, 0, st>>>(a, ld_a, b, ld_b, rowptr, perm, num_segments, dim, eps, p0, p1,
                                                         lse);
  if (num_elements > kChunkRows) {                     // else no segment is long
    const int tiles = (dim + CT - 1) / CT;
    const dim3 grid((unsigned)long_chunk_bound(num_elements), (unsigned)(tiles < kMaxTileGrid ? tiles : kMaxTileGrid));
    k_long<F, CT><<<grid, CT == 1 ? 128 : 256, 0, st>>>(a, ld_a, b, ld_b, rowptr, perm, num_segments, dim, chunk_start,
                                                        partial);
    const int64_t total = (int64_t)num_segments * dim;
    k_fold<F><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(partial, chunk_start, dim, total, eps, p0, p1, lse);
  }
}

template <typename F>
void launch_walk_ct(int ct, const float *a, int64_t ld_a, const float *b, int64_t ld_b, const int32_t *rowptr,
                    const int32_t *perm, int num_segments, int64_t num_elements, int dim, float eps, float *p0, float *p1,
                    float *lse, const int32_t *chunk_start, void *partial, hipStream_t st) {
#define SSM_WALK(CT_)                                                                                                 \
  launch_walk<F, CT_>(a, ld_a, b, ld_b, rowptr, perm, num_segments, num_elements, dim, eps, p0, p1, lse, chunk_start, \
                      partial, st)
  switch (ct) {
    case 1: SSM_WALK(1); break;
    case 2: SSM_WALK(2); break;
    case 4: SSM_WALK(4); break;
    case 8: SSM_WALK(8); break;
    case 16: SSM_WALK(16); break;
    case 32: SSM_WALK(32); break;
    default: SSM_WALK(64); break;
  }
#undef SSM_WALK
}

template <int MODE>
void launch_write(bool vec4, unsigned blocks, hipStream_t st, const float *a, int64_t ld_a, const float *b, int64_t ld_b,
                  const int64_t *index, const float *p0, const float *p1, int64_t num_segments, int64_t num_elements,
                  int dim, float *out, int64_t ld_out) {
  if (vec4)
    k_write<MODE, 4><<<blocks, kWriteThreads, 0, st>>>(a, ld_a, b, ld_b, index, p0, p1, num_segments, num_elements, dim,
                                                       out, ld_out);
  else
    k_write<MODE, 1><<<blocks, kWriteThreads, 0, st>>>(a, ld_a, b, ld_b, index, p0, p1, num_segments, num_elements, dim,
                                                       out, ld_out);
}

}  // namespace
}  // namespace ptgnn_amd

using namespace ptgnn_amd;

extern "C" int ptgnn_amd_segment_softmax_supported(int64_t num_segments, int64_t num_elements, int64_t dim) {
  return softmax_supported(num_segments, num_elements, dim) ? 1 : 0;
}

extern "C" size_t ptgnn_amd_segment_softmax_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                            int32_t fold) {
  if (!softmax_supported(num_segments, num_elements, dim) || num_segments == 0) return 0;
  return softmax_workspace(num_segments, num_elements, dim, fold).total;
}

extern "C" int ptgnn_amd_segment_softmax_state_f32(const float *a, int64_t ld_a, const float *b, int64_t ld_b,
                                                   const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                                   int64_t num_elements, int32_t dim, int32_t fold, float eps, float *p0,
                                                   float *p1, float *lse, void *workspace, size_t workspace_bytes,
                                                   void *stream_) {
  const char *what = "segment_softmax_state";
  PTGNN_REQUIRE(num_segments >= 0 && num_elements >= 0 && dim > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(fold == PTGNN_AMD_SSM_FOLD_MAXSUM || fold == PTGNN_AMD_SSM_FOLD_SUM || fold == PTGNN_AMD_SSM_FOLD_DOT,
                PTGNN_AMD_EINVAL, "%s: bad fold %d", what, fold);
  PTGNN_REQUIRE(softmax_supported(num_segments, num_elements, dim), PTGNN_AMD_EUNSUPPORTED,
                "%s: elements, segments and segments * dim must each stay below 2^31", what);
  if (num_segments == 0) return PTGNN_AMD_OK;
  const bool maxsum = fold == PTGNN_AMD_SSM_FOLD_MAXSUM, two = fold == PTGNN_AMD_SSM_FOLD_DOT;
  PTGNN_REQUIRE(rowptr && p0 && (!maxsum || p1) && (num_elements == 0 || (a && perm && (!two || b))), PTGNN_AMD_EINVAL,
                "%s: null pointer", what);
  PTGNN_REQUIRE(num_elements == 0 || (ld_a >= dim && (!two || ld_b >= dim)), PTGNN_AMD_EINVAL,
                "%s: bad leading dimension", what);
  const SoftmaxWorkspace ws = softmax_workspace(num_segments, num_elements, dim, fold);
  if (const int rc = workspace_check(what, workspace, workspace_bytes, ws.total)) return rc;
  hipStream_t st = (hipStream_t)stream_;
  int32_t *chunk_start = carved<int32_t>(workspace, ws.chunk_start);
  void *partial = carved<char>(workspace, ws.partial);
  if (num_elements > kChunkRows) {
    k_long_chunk_starts<<<1, 1024, 0, st>>>(rowptr, (int)num_segments, chunk_start);
    PTGNN_LAUNCH_CHECK();
  }
  const int ct = column_lanes(dim);
  if (maxsum)
    launch_walk_ct<FoldMaxSum>(ct, a, ld_a, b, ld_b, rowptr, perm, (int)num_segments, num_elements, dim, eps, p0, p1, lse,
                               chunk_start, partial, st);
  else if (two)
    launch_walk_ct<FoldDot>(ct, a, ld_a, b, ld_b, rowptr, perm, (int)num_segments, num_elements, dim, eps, p0, p1, lse,
                            chunk_start, partial, st);
  else
    launch_walk_ct<FoldSum>(ct, a, ld_a, b, ld_b, rowptr, perm, (int)num_segments, num_elements, dim, eps, p0, p1, lse,
                            chunk_start, partial, st);
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}

extern "C" int ptgnn_amd_segment_softmax_write_f32(const float *a, int64_t ld_a, const float *b, int64_t ld_b,
                                                   const int64_t *index, const float *p0, const float *p1,
                                                   int64_t num_segments, int64_t num_elements, int32_t dim, int32_t mode,
                                                   float *out, int64_t ld_out, void *stream_) {
  const char *what = "segment_softmax_write";
  PTGNN_REQUIRE(num_segments >= 0 && num_elements >= 0 && dim > 0, PTGNN_AMD_EINVAL, "%s: bad sizes", what);
  PTGNN_REQUIRE(mode >= PTGNN_AMD_SSM_LOG_SOFTMAX && mode <= PTGNN_AMD_SSM_LOGSUMEXP_BACKWARD, PTGNN_AMD_EINVAL,
                "%s: bad mode %d", what, mode);
  PTGNN_REQUIRE(softmax_supported(num_segments, num_elements, dim), PTGNN_AMD_EUNSUPPORTED,
                "%s: elements, segments and segments * dim must each stay below 2^31", what);
  if (num_elements == 0) return PTGNN_AMD_OK;
  const bool uses_b = mode == PTGNN_AMD_SSM_LOG_SOFTMAX_BACKWARD || mode == PTGNN_AMD_SSM_SOFTMAX_BACKWARD;
  const bool uses_p1 = !uses_b;
  PTGNN_REQUIRE(a && index && p0 && out && (!uses_b || b) && (!uses_p1 || p1), PTGNN_AMD_EINVAL, "%s: null pointer",
                what);
  PTGNN_REQUIRE(ld_a >= dim && ld_out >= dim && (!uses_b || ld_b >= dim), PTGNN_AMD_EINVAL, "%s: bad leading dimension",
                what);
  const bool vec4 = dim % 4 == 0 && ld_a % 4 == 0 && ld_out % 4 == 0 && aligned16(a) && aligned16(out) && aligned16(p0) &&
                    (!uses_b || (ld_b % 4 == 0 && aligned16(b))) && (!uses_p1 || aligned16(p1));
  const int64_t items = num_elements * (dim / (vec4 ? 4 : 1));
  const int64_t want = (items + kWriteThreads - 1) / kWriteThreads;
  const unsigned blocks = (unsigned)(want < kWriteMaxBlocks ? want : kWriteMaxBlocks);
  hipStream_t st = (hipStream_t)stream_;
#define SSM_WRITE(MODE_) \
  launch_write<MODE_>(vec4, blocks, st, a, ld_a, b, ld_b, index, p0, p1, num_segments, num_elements, dim, out, ld_out)
  switch (mode) {
    case PTGNN_AMD_SSM_LOG_SOFTMAX: SSM_WRITE(PTGNN_AMD_SSM_LOG_SOFTMAX); break;
    case PTGNN_AMD_SSM_SOFTMAX: SSM_WRITE(PTGNN_AMD_SSM_SOFTMAX); break;
    case PTGNN_AMD_SSM_LOG_SOFTMAX_BACKWARD: SSM_WRITE(PTGNN_AMD_SSM_LOG_SOFTMAX_BACKWARD); break;
    case PTGNN_AMD_SSM_SOFTMAX_BACKWARD: SSM_WRITE(PTGNN_AMD_SSM_SOFTMAX_BACKWARD); break;
    default: SSM_WRITE(PTGNN_AMD_SSM_LOGSUMEXP_BACKWARD); break;
  }
#undef SSM_WRITE
  PTGNN_LAUNCH_CHECK();
  return PTGNN_AMD_OK;
}
