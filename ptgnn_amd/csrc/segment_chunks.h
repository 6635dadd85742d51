// The chunk walk of a node -> graph plan, shared by weighted_pool.hip, attention_pool.hip, graph_norm.hip, segment_scores.hip
// and (the workgroup scan only) block_attention.hip.
//
// Segments are graphs: few and long.  Every segment of a plan is cut into CHUNKS OF kChunkRows ROWS COUNTED FROM THE
// SEGMENT'S OWN START; workgroup b works on one chunk, and a later launch adds the chunk partials of a segment IN CHUNK
// ORDER.  The chunk table says which chunk a workgroup has:
//     chunk_start[g] = chunks of the segments in front of g, chunk_start[G] = all chunks   (k_pool_chunk_starts)
//     workgroup b -> segment g with chunk_start[g] <= b < chunk_start[g + 1], rows rowptr[g] + 128 (b - chunk_start[g]) ..
// No float atomics: the value of a segment is a fixed function of ITS rows and their order, wherever the segment sits in
// the batch -- a graph pools / normalises to the same bits alone and inside a batch, which a sharded run that keeps whole
// graphs on a rank relies on.  That holds because every kernel cuts and folds by the ONE rule of this header.
//
// Workspaces.  An op describes its workspace once, as a function that carves offsets with `Carve` and returns them with
// the total; its *_workspace_bytes export and its entry point both call that function, so the two cannot disagree.
// Every block starts on a 256-byte boundary.  (The weighted pool's partial rows used to follow its chunk table without
// that padding: its workspace grew by up to 252 bytes when it moved here, the other sizes are what they were.)
#pragma once
#include "wave_ops.h"

namespace ptgnn_amd {

constexpr int kChunkRows = 128;   // rows of one chunk, counted from the start of its segment

// chunk b of the plan: its segment and the plan slots [lo, hi) of its rows
struct ChunkSpan {
  int seg, lo, hi;
};

// false for a workgroup past the last chunk (grids are the host's upper bound chunk_count_bound).  Workgroup-uniform.
__device__ __forceinline__ bool chunk_locate(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ chunk_start,
                                             int num_segments, int b, ChunkSpan &s) {
  if (b >= chunk_start[num_segments]) return false;
  s.seg = 0;
  int hi_seg = num_segments;                           // chunk_start[seg] <= b < chunk_start[seg + 1]
  while (hi_seg - s.seg > 1) {
    const int mid = (s.seg + hi_seg) >> 1;
    if (chunk_start[mid] <= b) s.seg = mid; else hi_seg = mid;
  }
  const int end = rowptr[s.seg + 1];
  s.lo = rowptr[s.seg] + (b - chunk_start[s.seg]) * kChunkRows;
  s.hi = s.lo + kChunkRows < end ? s.lo + kChunkRows : end;
  return true;
}

// p[c0 * stride], p[(c0 + 1) * stride], ... added in that order (four loads in flight, one chain of additions)
template <typename T>
__device__ __forceinline__ T chunk_fold(const T *__restrict__ p, int64_t stride, int c0, int c1) {
  T t = 0;
  int c = c0;
  for (; c + 4 <= c1; c += 4) {
    const T a0 = p[c * stride], a1 = p[(c + 1) * stride], a2 = p[(c + 2) * stride], a3 = p[(c + 3) * stride];
    t += a0; t += a1; t += a2; t += a3;
  }
  for (; c < c1; ++c) t += p[c * stride];
  return t;
}

// Running count over the segments of a plan by ONE workgroup of BLOCK threads, BLOCK segments per step: `__shared__
// SegmentScan<BLOCK> scan; scan.begin();` then, per step, every thread calls step(c) with the count of its segment (0 past
// the last) and gets the counts of all segments in front of it.  After a step, total() is the count so far.
template <int BLOCK>
struct SegmentScan {
  int wsum[BLOCK / 64];
  int carry;

  __device__ __forceinline__ void begin() {
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
  }

  __device__ __forceinline__ int step(int c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_inclusive_scan(c);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int run = carry + inc - c;
    for (int v = 0; v < wave; ++v) run += wsum[v];
    __syncthreads();
    if (threadIdx.x == BLOCK - 1) carry = run + c;
    __syncthreads();
    return run;
  }

  __device__ __forceinline__ int total() const { return carry; }
};

// upper bound of the chunks of a plan: the grid of every chunk kernel
inline int64_t chunk_count_bound(int64_t segments, int64_t elements) { return elements / kChunkRows + segments; }
inline size_t chunk_table_bytes(int64_t segments) { return (size_t)(segments + 1) * sizeof(int32_t); }

// the two launches every chunked op shares (defined in weighted_pool.hip)
void launch_chunk_starts(const int32_t *rowptr, int num_segments, int32_t *chunk_start, hipStream_t st);
// out[g, :dim] = partial rows chunk_start[g] .. chunk_start[g + 1] - 1 added in chunk order (0 for an empty segment)
void launch_fold_segments(const float *partial, const int32_t *chunk_start, int dim, int64_t segments, float *out,
                          int64_t ld_out, hipStream_t st);

// bump carver of a workspace: take() returns the offset of the next block, on a 256-byte boundary; `off` is the total
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = (off + 255) / 256 * 256;
    off = at + bytes;
    return at;
  }
};

template <typename T>
inline T *carved(void *workspace, size_t at) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + at); }

// The size checks the chunked entry points share: no negative size, and everything a kernel indexes with an int fits one
// (the chunk grid, the plan slots, and `per_segment` values per segment).  A plan without segments launches nothing and
// is not measured.  0 when fine; sets the error text with `what`.
inline int chunked_segments_check(const char *what, int64_t num_segments, int64_t num_elements, int32_t dim,
                                  int64_t per_segment = 1) {
  PTGNN_REQUIRE(num_segments >= 0 && num_elements >= 0 && dim > 0 && per_segment > 0, PTGNN_AMD_EINVAL, "%s: bad sizes",
                what);
  if (num_segments == 0) return PTGNN_AMD_OK;
  const int64_t lim = (int64_t)1 << 31;
  PTGNN_REQUIRE(chunk_count_bound(num_segments, num_elements) < lim && num_elements < lim &&
                    num_segments <= (lim - 1) / per_segment,      // num_segments * per_segment < 2^31, without the product
                PTGNN_AMD_EUNSUPPORTED, "%s: too many segments / elements", what);
  return PTGNN_AMD_OK;
}

inline int workspace_check(const char *what, const void *workspace, size_t have, size_t need) {
  PTGNN_REQUIRE(workspace && have >= need, PTGNN_AMD_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", what, have, need);
  return PTGNN_AMD_OK;
}

}  // namespace ptgnn_amd
