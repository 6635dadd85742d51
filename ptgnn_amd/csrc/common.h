// Shared helpers for libptgnn_amd (gfx950 only; no portability layer by design).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ptgnn_amd.h"

namespace ptgnn_amd {

void set_error(const char *fmt, ...);
void count_launch(int kernel_id);   // PTGNN_AMD_KERNEL_* of include/ptgnn_amd.h

#define PTGNN_REQUIRE(cond, code, ...)            \
  do {                                            \
    if (!(cond)) {                                \
      ::ptgnn_amd::set_error(__VA_ARGS__);        \
      return (code);                              \
    }                                             \
  } while (0)

#define PTGNN_HIP(expr)                                                                    \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      ::ptgnn_amd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                             __FILE__, __LINE__);                                          \
      return PTGNN_AMD_EHIP;                                                               \
    }                                                                                      \
  } while (0)

#define PTGNN_LAUNCH_CHECK()                                                               \
  do {                                                                                     \
    hipError_t _e = hipGetLastError();                                                     \
    if (_e != hipSuccess) {                                                                \
      ::ptgnn_amd::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),    \
                             __FILE__, __LINE__);                                          \
      return PTGNN_AMD_EHIP;                                                               \
    }                                                                                      \
  } while (0)

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kNumXcd = 8;       // MI355X: 8 XCDs, block b is observed on XCD b % 8

// XCD-aware tile order: consecutive tiles go to the SAME XCD (contiguous node ranges -- i.e. whole
// graphs of a disjoint-union batch -- share one 4 MiB L2), while hardware round-robins blockIdx
// over the XCDs.  Performance only; correctness never depends on placement.
__device__ __forceinline__ int64_t xcd_swizzle(int64_t block, int64_t nblocks) {
  const int64_t per = (nblocks + kNumXcd - 1) / kNumXcd;
  const int64_t tile = (block % kNumXcd) * per + block / kNumXcd;
  return tile;  // may be >= nblocks for the ragged tail: caller must bounds-check
}

inline int64_t xcd_padded_blocks(int64_t nblocks) {
  const int64_t per = (nblocks + kNumXcd - 1) / kNumXcd;
  return per * kNumXcd;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Segment pools cut every segment of a plan into chunks of kPoolChunkRows rows counted from the segment's own start and
// add the chunk partials in chunk order (weighted_pool.hip; attention_pool.hip uses the same chunk table and fold).
constexpr int kPoolChunkRows = 128;
int64_t pool_chunk_count_bound(int64_t segments, int64_t elements);   // upper bound of the chunks of a plan
size_t pool_chunk_table_bytes(int64_t segments);                     // int32 chunk_start[segments + 1], padded
// chunk_start[g] = chunks of the segments in front of g, chunk_start[G] = all chunks (one workgroup)
void launch_pool_chunk_starts(const int32_t *rowptr, int num_segments, int32_t *chunk_start, hipStream_t st);
// out[g, :dim] = partial rows chunk_start[g] .. chunk_start[g + 1] - 1 added in chunk order (0 for an empty segment)
void launch_fold_segments(const float *partial, const int32_t *chunk_start, int dim, int64_t segments, float *out,
                          int64_t ld_out, hipStream_t st);

}  // namespace ptgnn_amd
