// What projection_loss.hip takes from vocab_loss.hip: the second launch of the forward.  One copy of the merge, so the
// two routes fold their chunk partials, add the copy term and round the normaliser's (maximum, log of the sum) pair alike.
#pragma once
#include "common.h"

namespace ptgnn_amd {

// k_vocab_loss_merge (defined in vocab_loss.hip), a thread per row: partial [rows, chunks] the (max, sum) pairs of the
// column chunks of a row ((-inf, 0) for a chunk without a finite score), folded in chunk order; target_score [rows]
// holds s[r, targets[r]] for every row whose target lies in [0, vocab).  Writes norm, picked (with targets) and stats.
void launch_vocab_loss_merge(const float2 *partial, const float *target_score, int64_t rows, int32_t vocab, int chunks,
                             const float *extra, const int64_t *targets, float *norm, float *picked, float2 *stats,
                             hipStream_t st);

}  // namespace ptgnn_amd
