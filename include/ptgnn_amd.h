/*
 * ptgnn_amd -- MI355X (gfx950 / CDNA4) message-passing core for microsoft/ptgnn.
 *
 * C ABI of libptgnn_amd.so.  The reference (100 % Python) has no FFI of its own for this path;
 * its device work is delegated to `torch` and the third-party `torch_scatter` wheel.  Each entry
 * point below names the reference call site(s) (paths relative to the ptgnn checkout) whose
 * device work it replaces.  INTEGRATION.md shows the ctypes binding a ptgnn maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is documented "host";
 *   - the library never allocates, frees or retains user-visible memory: outputs and
 *     workspaces are caller-owned (in the Python host they are torch tensors, so the caching
 *     allocator, streams and graph capture keep working);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); no entry point
 *     synchronises the host;
 *   - return value: 0 = ok, <0 = PTGNN_AMD_E*; ptgnn_amd_last_error() returns a thread-local
 *     message for the last failure on the calling thread;
 *   - fp32 row-major matrices; a leading dimension `ld*` is counted in floats;
 *   - entry points are re-entrant: any number of host threads may call them concurrently, on the
 *     same or on different streams.  What the library keeps per process, and how it is guarded:
 *       * an immutable device-property cache and the per-(kernel, device) dynamic-LDS attribute
 *         (hipFuncSetAttribute, set once under a mutex; not legal inside a stream capture, so the
 *         first use of a streaming kernel has to happen outside one -- inside, the call falls back to
 *         the tile kernel or, where there is none, returns EUNSUPPORTED);
 *       * side streams + fork / join events of the aggregation (plans of >= 2 M edges with hub rows):
 *         one set per (device, caller stream), created on first use outside a capture, looked up and
 *         used under mutexes -- two caller streams never share an event; at most 64 sets, beyond that
 *         the launches stay on the caller's stream;
 *       * launch counters (ptgnn_amd_launch_count): relaxed atomics, never read by the library;
 *       * two TEST / DEVELOPER switches, process-wide on purpose (a torch backward runs on autograd worker threads,
 *         which have to see the setting of the thread that built the graph): ptgnn_amd_set_gemm_mode (which of two
 *         kernel families with identical bits serves the dense blocks) and ptgnn_amd_set_plan_path (which record
 *         format the plan build uses at small sizes).  RESULTS NEVER DEPEND ON EITHER -- they exist so that the
 *         parity tests can drive every kernel family / sort path on every shape; relaxed atomics, safe to flip
 *         between calls, not meant for production code (two models in one process simply share the default:
 *         dispatch by shape).  Environment variables
 *         (PTGNN_AMD_*) are read per call or once at first use; they are developer / test switches.
 *     Caller-owned state with an ownership rule: the plan build's `control` block and the hub
 *     `hub_tickets` counters are ZERO AT REST and belong to the launches of ONE stream at a time --
 *     give every stream that builds plans / aggregates concurrently its own.
 */
#ifndef PTGNN_AMD_H_
#define PTGNN_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden; the declarations of this header are its ONLY exported
 * symbols (`nm -D --defined-only libptgnn_amd.so` lists ptgnn_amd_* and nothing else). */
#pragma GCC visibility push(default)

/* 101: ptgnn_amd_shard_index gained `bad_index_count` (round 4, mid-signature); the fused aggregation + node-update
 * entry point ptgnn_amd_gather_update_f32 was added (round 5).  102: ptgnn_amd_weighted_pool*_f32 (round 6).
 * Callers check ptgnn_amd_version() >= the version their header was compiled against (the Python host does,
 * ptgnn_amd/_lib.py). */
#define PTGNN_AMD_VERSION 102 /* 0.1.2 */

enum {
  PTGNN_AMD_OK = 0,
  PTGNN_AMD_EINVAL = -1,       /* bad argument (null pointer, negative size, bad enum)         */
  PTGNN_AMD_EUNSUPPORTED = -2, /* shape outside what the kernels were built for                 */
  PTGNN_AMD_EHIP = -3,         /* a HIP runtime call or launch failed                           */
  PTGNN_AMD_EWORKSPACE = -4,   /* workspace too small                                           */
  PTGNN_AMD_ERANGE = -5        /* an index was out of [0, num_nodes) (only from *_validate)     */
};

/* reduce: the `aggregation_fn` strings accepted by AbstractMessagePassingLayer._aggregate_messages
 * (ptgnn/neuralmodels/gnn/messagepassing/abstractmessagepassing.py:38-50 -> torch_scatter.scatter):
 * "sum"/"add" = 0, "mean" = 1, "max" = 2, "min" = 3.  Empty segments yield 0 for every mode. */
enum { PTGNN_AMD_SUM = 0, PTGNN_AMD_MEAN = 1, PTGNN_AMD_MAX = 2, PTGNN_AMD_MIN = 3 };

/* Row epilogue fused into the aggregation kernel (MlpMessagePassingLayer,
 * mlpmessagepassing.py:114-117 + :56-58): message activation GELU (exact erf) and LayerNorm. */
enum { PTGNN_AMD_EPI_NONE = 0, PTGNN_AMD_EPI_GELU = 1, PTGNN_AMD_EPI_LAYERNORM = 2,
       PTGNN_AMD_EPI_GELU_LAYERNORM = 3 };

/* activation fused into ptgnn_amd_linear_f32 */
enum { PTGNN_AMD_ACT_NONE = 0, PTGNN_AMD_ACT_TANH = 1, PTGNN_AMD_ACT_RELU = 2 };

int ptgnn_amd_version(void);
const char *ptgnn_amd_last_error(void);

/* TEST / DEVELOPER switch (see "Conventions"): kernel family of the dense blocks (ptgnn_amd_linear_f32,
 * ptgnn_amd_gru_cell*_f32, ptgnn_amd_edge_linear_f32) -- i.e. of what replaces nn.Linear / nn.GRUCell at
 * gatedmessagepassing.py:57-69 and mlpmessagepassing.py:96-117.  Process-wide; initial value from the
 * environment variable PTGNN_AMD_GEMM (default 1).
 *   0  128 x 128 tile kernels, exact fp32 MFMA
 *   1  streaming weight-stationary kernels, exact fp32 MFMA (v_mfma_f32_32x32x2_f32: an fmaf chain)
 * Both produce the same bits (one K accumulation order); shapes the streaming kernels do not tile run on mode 0.
 * (Mode 2 of rounds 2-4 -- f32 emulated by a 3 x bf16 operand split -- was removed in round 5; it answers EINVAL.) */
int ptgnn_amd_set_gemm_mode(int mode);
int ptgnn_amd_get_gemm_mode(void);

/* ------------------------------------------------------------------------------------------
 * Which kernel family served a call is decided per call from shape, size and GEMM mode (the streaming
 * kernels take widths that are multiples of 64 and, for `linear`, enough rows to fill the chip).
 * ptgnn_amd_launch_count(id) returns how many launches of family `id` this process has made
 * (host-side relaxed counters; tests take differences around a call to assert the dispatch);
 * ptgnn_amd_launch_name(id) names it (NULL past the last id).
 * PTGNN_AMD_FORCE_STREAM=1 in the environment (read per call) lifts the SIZE thresholds of the
 * streaming `linear` dispatch, so that small reference fixtures can be replayed on it.
 * ---------------------------------------------------------------------------------------- */
enum {
  PTGNN_AMD_KERNEL_STREAM_LINEAR = 0,
  PTGNN_AMD_KERNEL_STREAM_LINEAR_RING,
  PTGNN_AMD_KERNEL_STREAM_GRU,
  PTGNN_AMD_KERNEL_STREAM_GRU_RING,
  PTGNN_AMD_KERNEL_STREAM_EDGE,
  PTGNN_AMD_KERNEL_STREAM_EDGE_SHARED,
  PTGNN_AMD_KERNEL_STREAM_EDGE_V2,
  PTGNN_AMD_KERNEL_WGRAD_STREAM,
  PTGNN_AMD_KERNEL_TILE_LINEAR,
  PTGNN_AMD_KERNEL_TILE_GRU,
  PTGNN_AMD_KERNEL_TILE_EDGE,
  PTGNN_AMD_KERNEL_TILE_WGRAD,
  PTGNN_AMD_KERNEL_GATHER_UPDATE,
  PTGNN_AMD_KERNEL_COUNT_
};
/* A second id range for the aggregation kernels (not reached by walking ids 0, 1, ... up to the first NULL name, so
 * the GEMM family list above stays as it is); ptgnn_amd_launch_count / _name take these ids too. */
enum {
  PTGNN_AMD_KERNEL_AGG_FIRST_ = 64,
  PTGNN_AMD_KERNEL_GATHER_REDUCE = PTGNN_AMD_KERNEL_AGG_FIRST_, /* ptgnn_amd_gather_reduce_f32 / _rows_f32 */
  PTGNN_AMD_KERNEL_EGC_GATHER_COMBINE,
  PTGNN_AMD_KERNEL_EGC_COMBINE,
  PTGNN_AMD_KERNEL_EGC_COMBINE_BACKWARD,
  PTGNN_AMD_KERNEL_PNA_AGGREGATE,          /* ptgnn_amd_pna_aggregate_f32 */
  PTGNN_AMD_KERNEL_PNA_AGGREGATE_BACKWARD, /* ptgnn_amd_pna_aggregate_backward_f32 */
  PTGNN_AMD_KERNEL_ATTENTION_POOL,          /* ptgnn_amd_attention_pool_f32 */
  PTGNN_AMD_KERNEL_ATTENTION_POOL_BACKWARD, /* ptgnn_amd_attention_pool_backward_f32 */
  PTGNN_AMD_KERNEL_HEAD_PROJECTION,         /* ptgnn_amd_head_projection_f32 */
  PTGNN_AMD_KERNEL_GRAPH_NORM,              /* ptgnn_amd_graph_norm_f32 */
  PTGNN_AMD_KERNEL_GRAPH_NORM_BACKWARD,     /* ptgnn_amd_graph_norm_backward_f32 */
  PTGNN_AMD_KERNEL_BLOCK_ATTENTION,          /* ptgnn_amd_block_attention_f32 */
  PTGNN_AMD_KERNEL_BLOCK_ATTENTION_BACKWARD, /* ptgnn_amd_block_attention_backward_f32 */
  PTGNN_AMD_KERNEL_SEGMENT_SCORES,           /* ptgnn_amd_segment_scores_f32 */
  PTGNN_AMD_KERNEL_SEGMENT_SCORES_BACKWARD,  /* ptgnn_amd_segment_scores_backward_f32 */
  PTGNN_AMD_KERNEL_EMBEDDING_BAG,            /* ptgnn_amd_embedding_bag_f32 */
  PTGNN_AMD_KERNEL_EMBEDDING_BAG_BACKWARD,   /* ptgnn_amd_embedding_bag_backward_f32 */
  PTGNN_AMD_KERNEL_AGG_END_
};
/* A third id range, past the aggregation range for the same reason: the kernels of the char-CNN embedder
 * (csrc/char_conv.hip).  Its windowed GEMMs count under the GEMM families above. */
enum {
  PTGNN_AMD_KERNEL_CHAR_FIRST_ = 128,
  PTGNN_AMD_KERNEL_CHAR_EMBED = PTGNN_AMD_KERNEL_CHAR_FIRST_, /* ptgnn_amd_char_embed_f32 */
  PTGNN_AMD_KERNEL_CHAR_EMBED_BACKWARD,                       /* ptgnn_amd_char_embed_backward_f32 */
  PTGNN_AMD_KERNEL_WINDOW_MAX,                                /* ptgnn_amd_window_max_f32 */
  PTGNN_AMD_KERNEL_WINDOW_MAX_BACKWARD,                       /* ptgnn_amd_window_max_backward_f32 */
  PTGNN_AMD_KERNEL_CHAR_END_
};
/* A fourth id range: the task heads (csrc/task_heads.hip).  Their Linears count under the GEMM families above. */
enum {
  PTGNN_AMD_KERNEL_HEAD_FIRST_ = 192,
  PTGNN_AMD_KERNEL_LOGIT_LOSS = PTGNN_AMD_KERNEL_HEAD_FIRST_, /* ptgnn_amd_logit_loss_f32 */
  PTGNN_AMD_KERNEL_LOGIT_LOSS_BACKWARD,                       /* ptgnn_amd_logit_loss_backward_f32 */
  PTGNN_AMD_KERNEL_CANDIDATE_SCORES,                          /* ptgnn_amd_candidate_scores_f32 */
  PTGNN_AMD_KERNEL_CANDIDATE_SCORES_BACKWARD,                 /* ptgnn_amd_candidate_scores_backward_f32 */
  PTGNN_AMD_KERNEL_HEAD_END_
};
/* A fifth id range: the loss of the copying decoder (csrc/vocab_loss.hip). */
enum {
  PTGNN_AMD_KERNEL_SEQ_FIRST_ = 256,
  PTGNN_AMD_KERNEL_VOCAB_LOSS = PTGNN_AMD_KERNEL_SEQ_FIRST_, /* ptgnn_amd_vocab_loss_f32 */
  PTGNN_AMD_KERNEL_VOCAB_LOSS_BACKWARD,                      /* ptgnn_amd_vocab_loss_backward_f32 */
  PTGNN_AMD_KERNEL_COPY_LOSS_FINISH,                         /* ptgnn_amd_copy_loss_finish_f32 */
  PTGNN_AMD_KERNEL_SEQ_END_
};
/* A sixth id range: the greedy-decoding step of the copying decoder (csrc/decode_step.hip). */
enum {
  PTGNN_AMD_KERNEL_DECODE_FIRST_ = 320,
  PTGNN_AMD_KERNEL_DECODE_STEP = PTGNN_AMD_KERNEL_DECODE_FIRST_, /* ptgnn_amd_decode_step_f32 */
  PTGNN_AMD_KERNEL_DECODE_END_
};
/* A seventh id range: the beam-search step of the copying decoder (csrc/beam_step.hip; its two kernels count as one). */
enum {
  PTGNN_AMD_KERNEL_BEAM_FIRST_ = 384,
  PTGNN_AMD_KERNEL_BEAM_STEP = PTGNN_AMD_KERNEL_BEAM_FIRST_, /* ptgnn_amd_beam_step_f32 */
  PTGNN_AMD_KERNEL_BEAM_END_
};
/* An eighth id range: the opt-in 16-bit-input dense blocks (csrc/half_gemm.hip). */
enum {
  PTGNN_AMD_KERNEL_HALF_FIRST_ = 448,
  PTGNN_AMD_KERNEL_HALF_LINEAR = PTGNN_AMD_KERNEL_HALF_FIRST_, /* ptgnn_amd_half_linear */
  PTGNN_AMD_KERNEL_HALF_GRU,                                   /* ptgnn_amd_half_gru_cell */
  PTGNN_AMD_KERNEL_HALF_END_
};
/* A ninth id range: the opt-in 16-bit-input grouped per-edge GEMM (csrc/edge_gemm16.hip). */
enum {
  PTGNN_AMD_KERNEL_EDGE16_FIRST_ = 512,
  PTGNN_AMD_KERNEL_EDGE16 = PTGNN_AMD_KERNEL_EDGE16_FIRST_, /* ptgnn_amd_edge_linear16 */
  PTGNN_AMD_KERNEL_EDGE16_SHARED,                           /* ptgnn_amd_edge_linear16_shared */
  PTGNN_AMD_KERNEL_EDGE16_END_
};
/* A tenth id range: the opt-in 16-bit-input TRAINING launches (csrc/wgrad16.hip, csrc/half_gemm.hip).  A range of its
 * own, so the eighth range ends where it did. */
enum {
  PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_ = 576,
  PTGNN_AMD_KERNEL_HALF_WGRAD = PTGNN_AMD_KERNEL_HALF_TRAIN_FIRST_, /* ptgnn_amd_linear_weight_grad16 */
  PTGNN_AMD_KERNEL_HALF_GRU_TRAIN,                                  /* ptgnn_amd_gru_cell_train16 */
  PTGNN_AMD_KERNEL_HALF_LINEAR_ADD,                                 /* ptgnn_amd_linear_add16 */
  PTGNN_AMD_KERNEL_HALF_TRAIN_END_
};
/* An eleventh id range: the 16-bit-input grouped per-edge GEMM WITH a target-state half (csrc/edge_gemm16.hip: the MLP-MP
 * message Linear).  A range of its own, so the ninth range ends where it did. */
enum {
  PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_ = 640,
  PTGNN_AMD_KERNEL_EDGE16_DST = PTGNN_AMD_KERNEL_EDGE16_DST_FIRST_, /* ptgnn_amd_edge_dst_linear16 */
  PTGNN_AMD_KERNEL_EDGE16_DST_END_
};
/* A twelfth id range: the finishing route of the beam search (csrc/beam_step.hip: the step that writes back-pointer pairs,
 * its two kernels counted as one, and the backtrack).  A range of its own, so the seventh range ends where it did. */
enum {
  PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_ = 704,
  PTGNN_AMD_KERNEL_BEAM_STEP_LINKS = PTGNN_AMD_KERNEL_BEAM_FINISH_FIRST_, /* ptgnn_amd_search_step_links_f32 */
  PTGNN_AMD_KERNEL_BEAM_BACKTRACK,                                        /* ptgnn_amd_search_backtrack */
  PTGNN_AMD_KERNEL_BEAM_FINISH_END_
};
/* A thirteenth id range: the 16-bit-input forward of the block attention (csrc/block_attention16.hip).  A range of its
 * own, so the second range ends where it did. */
enum {
  PTGNN_AMD_KERNEL_ATTENTION16_FIRST_ = 768,
  PTGNN_AMD_KERNEL_BLOCK_ATTENTION16 = PTGNN_AMD_KERNEL_ATTENTION16_FIRST_, /* ptgnn_amd_attention16_block */
  PTGNN_AMD_KERNEL_ATTENTION16_END_
};
/* A fourteenth id range: the 16-bit-input launches of the GGNN edge-form TRAINING step (csrc/edge_gemm16.hip's masked
 * forms, csrc/edge_wgrad16.hip).  A range of its own, so the ninth and tenth ranges end where they did. */
enum {
  PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_ = 832,
  PTGNN_AMD_KERNEL_EDGE16_MASKED = PTGNN_AMD_KERNEL_EDGE16_TRAIN_FIRST_, /* ptgnn_amd_edge_masked_linear16, modes 1, 2 */
  PTGNN_AMD_KERNEL_EDGE_WGRAD16,                                         /* ptgnn_amd_edge_weight_grad16 */
  PTGNN_AMD_KERNEL_EDGE16_TRAIN_END_
};
int64_t ptgnn_amd_launch_count(int kernel_id);
const char *ptgnn_amd_launch_name(int kernel_id);

/* ------------------------------------------------------------------------------------------
 * Graph plan: merge the per-edge-type adjacency lists of one minibatch into ONE
 * destination-sorted CSR that all L message-passing layers of a forward reuse.
 *
 * Replaces: `torch.cat([adj[1] ...])` + the per-type Python loop + the unsorted scatter index
 *   (gatedmessagepassing.py:46,50-64; mlpmessagepassing.py:81-112) -- the adjacency is the same
 *   for every layer (graphneuralnetwork.py:122-131), so the sort is paid once per batch.
 *
 * Input : num_types pairs of int64 device arrays (exactly the tensors ptgnn's
 *         GraphNeuralNetworkModel.finalize_minibatch produces, graphneuralnetwork.py:461-467),
 *         given as HOST arrays of device pointers + HOST array of lengths.
 * Output: rowptr[num_nodes+1]; for CSR slot i (in-edges of node v occupy
 *         rowptr[v]..rowptr[v+1], in the reference's message order = type-major, then edge
 *         order, i.e. the sort is STABLE so fp32 sums fold in the same order as the CPU path):
 *           col[i]  = (src << type_bits) | edge_type     (type_bits = ceil(log2(num_types)))
 *           perm[i] = position of the edge in the type-major concatenation (nullable)
 * `num_src_rows` = number of rows of the table the sources index (0 = num_nodes); it exceeds
 * num_nodes for a dst-range shard whose sources include halo rows (ptgnn_amd/sharded.py).
 * Requires num_src_rows << type_bits < 2^31 and num_edges < 2^31, else EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_csr_workspace_bytes(int64_t num_edges, int64_t num_nodes);
size_t ptgnn_amd_csr_control_bytes(void);
/* Test / A-B knob of the plan build (process-wide; results never depend on it): 0 = pick the record format by
 * size (default), 1 = force the 12-byte records + wide buckets of the large-graph path, 2 = additionally force
 * one LSD pre-pass (the > 21 row-bit path) -- so the parity tests can drive every path at sizes the numpy
 * argsort oracle finishes in seconds. */
int ptgnn_amd_set_plan_path(int path);
int ptgnn_amd_type_bits(int32_t num_types);
int ptgnn_amd_csr_build(const int64_t *const *src_per_type, /* host [num_types] of device ptrs */
                        const int64_t *const *dst_per_type, /* host [num_types] of device ptrs */
                        const int64_t *edges_per_type,      /* host [num_types]                */
                        int32_t num_types, int64_t num_nodes, int64_t num_src_rows,
                        int swap_src_dst, /* 0: rows = dst, col = (src << type_bits) | type          *
                                           * 1: rows = src, col = (dst << type_bits) | type          *
                                           * 2: rows = src * num_types + type, col = dst; pass       *
                                           *    num_nodes = source rows * num_types (backward plan)  */
                        int32_t *rowptr, int32_t *col, int32_t *perm /* nullable */,
                        int32_t *max_degree /* nullable device scalar: longest row */,
                        int32_t hub_threshold /* 0 = no hub list */,
                        int32_t *hub_entries /* nullable: int32 [2 * ceil(E/1024)][2] (chunk,row) */,
                        int32_t *hub_count /* nullable device scalar: number of pairs */,
                        int32_t *bad_index_count /* nullable device scalar, ACCUMULATED (never reset here):   *
                                                  * ids outside [0, num_nodes) / [0, num_src_rows) -- the     *
                                                  * reference device-asserts on those in F.embedding          *
                                                  * (gatedmessagepassing.py:54-56); here they are clamped to *
                                                  * row 0 so nothing is read or written out of bounds, and   *
                                                  * counted so the host can raise                            */,
                        void *control /* nullable: ptgnn_amd_csr_control_bytes() of device memory that is ZERO  *
                                       * AT REST: zero-filled once by the caller, used by the builds of ONE   *
                                       * stream at a time, left zero-filled by every build (digit totals and  *
                                       * tile counters of the three-launch build).  Null: the library zeroes  *
                                       * a block inside `workspace` with one extra memset per build          */,
                        void *workspace, size_t workspace_bytes, void *stream);

/* The hub (chunk, row) list of an existing rowptr (plans that are not built by ptgnn_amd_csr_build,
 * e.g. pooling over the already sorted node_to_graph_idx).  *hub_count must be 0 on entry. */
int ptgnn_amd_hub_list(const int32_t *rowptr, int64_t num_rows, int32_t hub_threshold,
                       int32_t *hub_entries, int32_t *hub_count, void *stream);

/* Optional debug aid (the reference performs no range check either): counts indices outside
 * [0, num_nodes) into *bad_count (device int32, caller zeroes it). */
int ptgnn_amd_validate_indices(const int64_t *idx, int64_t n, int64_t num_nodes,
                               int32_t *bad_count, void *stream);

/* ------------------------------------------------------------------------------------------
 * Index bookkeeping of a destination-range shard (north star: "large batched graphs shard by destination-node
 * range across up to 8 GPUs"; SURVEY.md 8e, 8f-3 "halo send lists").  The reference has no counterpart -- its only
 * multi-GPU mode is whole-batch data parallelism (distributedtrainer.py:250-297); the tensors it starts from are
 * the per-type int64 adjacency lists of finalize_minibatch (graphneuralnetwork.py:461-467), here in GLOBAL node ids
 * and restricted to the edges whose destination this rank owns ([lo, hi)).
 *   local_dst[e] = dst - lo;  local_src[e] = src - lo for an own source, else n_local + the source's slot in the
 *   sorted list of DISTINCT remote sources `need_ids` (ascending global ids = grouped by owner, because the
 *   ranges bounds[0] <= ... <= bounds[world] are ordered by rank); edges in the type-major order of the lists.
 *   stats (device int64 [world + 2 + num_types], zeroed here): [0, world) halo rows per owner |
 *   [world] edges with a remote source | [world + 1] halo rows in all | then own-source edges per edge type.
 * need_capacity >= min(num_edges, total_nodes - (hi - lo)).  Nothing synchronises with the host.
 * A source id outside [0, total_nodes) is clamped into the id space and COUNTED in *bad_index_count (after the remap
 * it would be an ordinary own / halo row: the plan build's range guard cannot see it any more); a destination
 * outside [lo, hi) leaves as a local id outside [0, hi - lo), which ptgnn_amd_csr_build counts.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_shard_index_workspace_bytes(int64_t total_nodes);
int ptgnn_amd_shard_index(const int64_t *const *src_per_type, const int64_t *const *dst_per_type,
                          const int64_t *edges_per_type, int32_t num_types, int64_t lo, int64_t hi,
                          const int64_t *bounds /* device [world + 1] */, int32_t world, int64_t total_nodes,
                          int64_t *local_src, int64_t *local_dst, int64_t *need_ids, int64_t need_capacity,
                          int64_t *stats,
                          int32_t *bad_index_count /* nullable; device int32, NOT zeroed here: += number of
                                                    * global source ids outside [0, total_nodes) (they are
                                                    * clamped; the reference device-asserts on them) */, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Unique (edge type, source) pairs of a forward plan.  A GGNN message is W_t . x[src]
 * (gatedmessagepassing.py:52-58: index_select of the source states, then the type's bias-free Linear): edges of one
 * type that leave the same node carry the SAME message row, so the grouped per-edge GEMM only has to produce one row
 * per pair that occurs and the aggregation reads it through slot_row.  Integer bookkeeping over the plan's col array
 * (ptgnn_amd_csr_build, mode 0); the values of the layer do not change.
 *   unique_src [capacity >= min(num_edges, num_src_rows * num_types)]: source node of every message row -- rows are
 *       type-major, ascending in the source id inside a type (so unique_src + the prefix of counts IS the adjacency
 *       input of ptgnn_amd_edge_linear_f32 for the de-duplicated launch);
 *   counts (device int64 [num_types + 1]): rows per edge type, [num_types] = rows in all;
 *   slot_row (int32 [num_edges]): message row of every CSR slot (the `col` argument of ptgnn_amd_gather_reduce_f32
 *       with type_bits = 0, where the per-edge form passes the plan's perm).
 * Nothing synchronises with the host.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_unique_sources_workspace_bytes(int64_t num_src_rows, int32_t num_types);
size_t ptgnn_amd_edge_table_bytes(void);
int ptgnn_amd_unique_sources(const int32_t *col, int64_t num_edges, int32_t type_bits, int32_t num_types,
                             int64_t num_src_rows, int32_t *slot_row, int64_t *unique_src, int64_t capacity,
                             int64_t *counts, void *edge_table /* nullable; ptgnn_amd_edge_table_bytes() */,
                             void *workspace, size_t workspace_bytes, void *stream);
/* The grouped per-edge GEMM of ptgnn_amd_edge_linear_f32 (no target-state half) over the message rows of
 * ptgnn_amd_unique_sources: msg[r] = act(W_t x[unique_src[r]]) for the rows r of edge type t.  How many rows each type
 * has is only known on the device, so the launch geometry (rows, 32-row units and workgroups per edge type) is read from
 * `edge_table`, which ptgnn_amd_unique_sources filled on the same stream -- the host never waits for the counts.
 * msg must hold min(num_edges, num_src_rows * num_types) rows.  PTGNN_AMD_EUNSUPPORTED for shapes outside the streaming
 * edge GEMM (ptgnn_amd_edge_linear_shared_supported == 0: the caller keeps the per-edge form). */
int ptgnn_amd_edge_linear_shared_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types);
int ptgnn_amd_edge_linear_shared_f32(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                     const void *edge_table, const float *const *w_per_type, int32_t num_types,
                                     int32_t msg_dim, int act, float *msg, int64_t ld_msg, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused gather -> (+ destination term) -> segment reduce -> (row epilogue).
 *
 *   out[v, :] = EPI( REDUCE_{i in rowptr[v]..rowptr[v+1]}  Ysrc[src_i, t_i*M : (t_i+1)*M]
 *                                                         (+ Ydst[v,   t_i*M : (t_i+1)*M]) )
 *   with (src_i, t_i) unpacked from col[i].
 *
 * Replaces, for one layer: F.embedding gathers, torch.cat, the per-type Linear outputs being
 *   materialised as [E, M], torch.cat of messages/targets and torch_scatter.scatter
 *   (gatedmessagepassing.py:54-68; mlpmessagepassing.py:88-112; abstractmessagepassing.py:44-50),
 *   using  Linear_t(x_src) == (X W_t^T)[src]  (bias-free Linear commutes with the row gather),
 *   and for MLP-MP with target state  W_t [x_u ; x_v] = W_t^s x_u + W_t^d x_v.
 *
 *   ysrc : [num_src_rows, ld_y] ; block t of M columns holds X W_t^T.  With type_bits == 0 and
 *          ld_y == M this is also the plain segment reduce of a materialised message matrix
 *          (col = perm), i.e. the torch_scatter seam itself.
 *   ydst : nullable, same column layout with its own leading dimension, indexed by the
 *          DESTINATION node.
 *   argout: nullable int32 [num_nodes, M]; for max/min the winning CSR slot, -1 if empty
 *          (backward routing; torch_scatter's arg_out).
 *   ln_gamma/ln_beta: LayerNorm affine parameters (EPI_*LAYERNORM only).
 *
 * Hub rows (power-law graphs): rows with more than `hub_threshold` in-edges (0 = never; otherwise
 * >= 2048 and equal to the threshold given to ptgnn_amd_csr_build) are split over 1024-slot chunks:
 * one small extra launch walks the plan's (chunk, row) list `hub_entries`/`hub_count`; the last
 * chunk of a hub to arrive folds the chunk partials in order and applies the epilogue, so one
 * 10^5-edge destination does not serialise on one lane group.  Needs `hub_ws` of
 * ptgnn_amd_hub_workspace_bytes(num_edges, msg_dim, argout != 0) bytes (scratch) and `hub_tickets`,
 * int32[ptgnn_amd_hub_ticket_count(num_edges, msg_dim)] that is ZERO on entry (the kernel leaves it
 * zero again, so one zeroed buffer per plan AND STREAM serves every call on that stream: two streams
 * aggregating over one plan concurrently need a buffer each); with either NULL every
 * row takes the serial path.  Deterministic; a hub row's fp32 fold order differs from the serial
 * order (max/min and argout are exact).
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_hub_workspace_bytes(int64_t num_edges, int32_t msg_dim, int with_arg);
int64_t ptgnn_amd_hub_ticket_count(int64_t num_edges, int32_t msg_dim);
int ptgnn_amd_gather_reduce_f32(const float *ysrc, int64_t ld_ysrc,
                                const float *ydst /* nullable */, int64_t ld_ydst,
                                const int32_t *rowptr, const int32_t *col,
                                int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                int reduce, int epilogue, const float *ln_gamma,
                                const float *ln_beta, float ln_eps, float *out, int64_t ld_out,
                                int32_t *argout /* nullable */, int64_t num_edges,
                                int32_t hub_threshold, const int32_t *hub_entries /* nullable */,
                                const int32_t *hub_count /* nullable */, void *hub_ws /* nullable */,
                                size_t hub_ws_bytes, int32_t *hub_tickets /* nullable */,
                                void *stream);
/* The same aggregation for the destination rows [row_begin, row_end) only (every pointer and count keeps its
 * whole-plan meaning; rows outside the range are neither read nor written, hub rows outside it are skipped).  A
 * layer's aggregation -> node update chain (gatedmessagepassing.py:63-69) is row-wise after the aggregation, so a
 * host MAY pipeline it over row ranges (the update of one range on one stream, the aggregation of the next on
 * another): ptgnn_amd.ops.aggregate_gru does, opt-in (PTGNN_AMD_AGG_PIPELINE=<ranges>; off by default -- it measured
 * slower than the unsplit pair on MI355X, profiles/r05_notes.md).  Launches over one plan must not overlap EACH OTHER
 * in time (they share `hub_tickets`). */
int ptgnn_amd_gather_reduce_rows_f32(const float *ysrc, int64_t ld_ysrc,
                                     const float *ydst /* nullable */, int64_t ld_ydst,
                                     const int32_t *rowptr, const int32_t *col,
                                     int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                     int reduce, int epilogue, const float *ln_gamma,
                                     const float *ln_beta, float ln_eps, float *out, int64_t ld_out,
                                     int32_t *argout /* nullable */, int64_t num_edges,
                                     int32_t hub_threshold, const int32_t *hub_entries /* nullable */,
                                     const int32_t *hub_count /* nullable */, void *hub_ws /* nullable */,
                                     size_t hub_ws_bytes, int32_t *hub_tickets /* nullable */,
                                     int64_t row_begin, int64_t row_end, void *stream);
/* Row headers: the first eight `col` entries of every destination row at an address that depends on the row alone.
 *   hdr int32 [num_rows, 8], 32-byte aligned:  hdr[r, k] = entries[min(rowptr[r] + k, rowptr[r + 1] - 1)]
 *   (slots past the row's end repeat its last entry -- the clamped duplicates the aggregation's groups of 8 load
 *   anyway); all zeros for an empty row, never read.  `entries` is whatever the aggregation will be given as `col`:
 *   the plan's col, its perm, or the slot_row of ptgnn_amd_unique_sources.  One launch, no host synchronisation.
 * ptgnn_amd_gather_reduce_hdr_f32 is ptgnn_amd_gather_reduce_rows_f32 with that array (`row_hdr`, nullable = the same
 * call): a lane group requests its row's record together with the rowptr pair and starts the first eight message
 * rows from it, so a row of up to eight in-edges is two dependent memory round trips instead of three (rowptr -> col
 * -> rows).  Later groups of a longer row read `col` as before.  Slots fold in the same order: the output bits do
 * not depend on `row_hdr`.  Used by the plain walks in groups of eight (16-byte-aligned rows, msg_dim <= 256, no
 * destination term, no argout); every other call ignores it.  Hub and long rows are left to their kernels as
 * without it. */
int ptgnn_amd_row_headers(const int32_t *rowptr, const int32_t *entries, int64_t num_rows, int32_t *hdr, void *stream);
int ptgnn_amd_gather_reduce_hdr_f32(const float *ysrc, int64_t ld_ysrc,
                                    const float *ydst /* nullable */, int64_t ld_ydst,
                                    const int32_t *rowptr, const int32_t *col,
                                    int32_t type_bits, int64_t num_nodes, int32_t msg_dim,
                                    int reduce, int epilogue, const float *ln_gamma,
                                    const float *ln_beta, float ln_eps, float *out, int64_t ld_out,
                                    int32_t *argout /* nullable */, int64_t num_edges,
                                    int32_t hub_threshold, const int32_t *hub_entries /* nullable */,
                                    const int32_t *hub_count /* nullable */, void *hub_ws /* nullable */,
                                    size_t hub_ws_bytes, int32_t *hub_tickets /* nullable */,
                                    int64_t row_begin, int64_t row_end,
                                    const int32_t *row_hdr /* nullable */, void *stream);

/* ------------------------------------------------------------------------------------------
 * MlpMessagePassingLayer, aggregation AND node update in one launch (mlpmessagepassing.py:107-117 with the update
 * network of :56-66):   out[v, :] = act(W . EPI(reduce over the CSR slots i of row v of msg[col[i] >> type_bits, :]) + b)
 * i.e. ptgnn_amd_gather_reduce_f32 (no destination term, no argout) followed by ptgnn_amd_linear_f32, bit for bit,
 * without the [num_nodes, msg_dim] aggregate ever existing in memory.  msg_dim must be 64 (the README's default
 * architecture; BASELINE config 4), out_dim a multiple of 32 up to 128: ptgnn_amd_gather_update_supported.  Every row
 * folds serially in slot order (no hub / long-row launches): meant for minibatch-sized plans.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_gather_update_supported(int32_t msg_dim, int32_t out_dim);
int ptgnn_amd_gather_update_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr, const int32_t *col,
                                int32_t type_bits, int64_t num_nodes, int32_t msg_dim, int reduce, int epilogue,
                                const float *ln_gamma /* nullable */, const float *ln_beta /* nullable */, float ln_eps,
                                const float *w /* [out_dim, msg_dim] */, const float *bias /* nullable */,
                                int32_t out_dim, int act, float *out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * reduce = "mul" of the scatter seam: abstractmessagepassing.py:44-50 hands the aggregation name to
 * torch_scatter.scatter, whose reduce set also holds "mul" (no shipped ptgnn configuration uses it).
 *   out[v, :] = product over the CSR slots i of row v of msg[perm[i], :], folded in slot order (= edge
 *   order: the plan's sort is stable); rows without in-edges are 1, like torch_scatter's scatter_mul
 *   (Reducer<MUL>::init(), no masked fill).  msg rows in the type-major message order, `perm` and
 *   `rowptr` from ptgnn_amd_csr_build.  Deterministic; a plain HBM-bound kernel (hub rows are serial).
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_segment_mul_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr, const int32_t *perm,
                              int64_t num_rows, int64_t num_edges, int32_t dim, float *out, int64_t ld_out,
                              void *stream);

/* Backward of the max/min aggregation w.r.t. the message table, over the BACKWARD plan (rows =
 * src * T + type, col = dst, built by ptgnn_amd_csr_build mode 2):
 *   out[r, c] = sum_{i in row r}  [ arg[col_i, c] == slot_of[i] ] * grad[col_i, c]
 * arg = the forward call's argout (winning forward CSR slot per (dst node, feature)); slot_of[i] = the
 * forward slot of backward slot i.  This is torch_scatter's "gradient flows to arg_out only"
 * rule (abstractmessagepassing.py:38-50 through torch_scatter's autograd) without materialising the
 * [E, M] per-edge gradient. */
int ptgnn_amd_gather_reduce_masked_f32(const float *grad, int64_t ld_grad, const int32_t *arg,
                                       const int32_t *rowptr, const int32_t *col,
                                       const int32_t *slot_of, int64_t num_rows, int32_t msg_dim,
                                       float *out, int64_t ld_out, int64_t num_edges,
                                       int32_t hub_threshold, const int32_t *hub_entries,
                                       const int32_t *hub_count, void *hub_ws /* nullable */,
                                       size_t hub_ws_bytes, int32_t *hub_tickets /* nullable */,
                                       void *stream);

/* ------------------------------------------------------------------------------------------
 * y = act(x W^T + b) on the matrix cores with exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces nn.Linear at gatedmessagepassing.py:20-23,57-61 (all T edge-type weights stacked
 * into one [T*M, H] matrix => ONE wide GEMM instead of T ragged ones), mlp.py:54-75,
 * mlpmessagepassing.py:60-63 (Linear + Tanh), residuallayers.py:112-116.
 *   x [rows, k] (ld_x), w [n_out, k] row-major contiguous (nn.Linear layout), bias nullable.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_linear_f32(const float *x, int64_t rows, int32_t k, int64_t ld_x, const float *w,
                         int32_t n_out, const float *bias, int act, float *y, int64_t ld_y,
                         void *stream);
/* y = act(x W^T + b) + addend, the add folded into the GEMM's store epilogue (training: the GRU cell's backward
 * `d_h + d_gh W_hh`, which torch ran as a separate pass over [N, H] per layer).  Streaming shapes only (K % 64 == 0,
 * n_out % 32 == 0, 16-byte aligned rows): others return PTGNN_AMD_EUNSUPPORTED without touching `y`. */
int ptgnn_amd_linear_add_f32(const float *x, int64_t rows, int32_t k, int64_t ld_x, const float *w, int32_t n_out,
                             const float *bias /* nullable */, int act, const float *addend, int64_t ld_add, float *y,
                             int64_t ld_y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Minibatch assembly on the device (GraphNeuralNetworkModel.extend_minibatch_with / finalize_minibatch,
 * graphneuralnetwork.py:386-493: per-graph `adj + nodes_in_mb_so_far`, np.concatenate, int64 tensors,
 * the node_to_graph_idx generator at :440-443): one launch turns the RAW per-graph int32 arrays
 * (one staging buffer) into every int64 index tensor of the minibatch.
 *   out[i] = (i < n_in ? in[i] : 0) + seg_add[s]   for  seg_start[s] <= i < seg_start[s+1]
 *   in int32 [n_in] device; seg_start int64 [num_segments + 1] (seg_start[0] = 0, last = n_out),
 *   seg_add int64 [num_segments]; out int64 [n_out].  Elements past n_in are "fill" segments
 *   (node_to_graph_idx, reference_node_graph_idx).  Bit-exact integer work.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_batch_offsets_i64(const int32_t *in, int64_t n_in, const int64_t *seg_start,
                                const int64_t *seg_add, int32_t num_segments, int64_t n_out,
                                int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-edge message GEMM, every edge type in ONE launch (grouped GEMM with gathered A rows):
 *   msg[off_t + e, :] = act( [ x[src_t[e], :] ; x[dst_t[e], :] (if dst_per_type) ] W_t^T ),  e < E_t
 * rows in the reference's message order (type-major, then edge order) = the matrix
 * `torch.cat(all_messages)` of gatedmessagepassing.py:50-64 / mlpmessagepassing.py:81-108, without the
 * F.embedding outputs, the torch.cat copies and the T per-type launches.  Cheaper than the per-node
 * pre-transform when E < N*T (many sparse edge types).  Feed the result to
 * ptgnn_amd_gather_reduce_f32 with col = perm, type_bits = 0.
 *   src/dst_per_type: HOST arrays of int64 device arrays (ptgnn's adjacency tensors); dst nullable.
 *   w_per_type: HOST array of device pointers to the per-type nn.Linear weights
 *               [msg_dim, state_dim * (dst ? 2 : 1)], row-major contiguous.
 * Requires state_dim % 32 == 0, msg_dim % 4 == 0, 16-byte aligned rows (else EUNSUPPORTED).
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_edge_linear_f32(const float *x, int64_t ld_x,
        int64_t num_rows /* rows of x: gathered node ids are clamped into [0, num_rows) */,
        int32_t state_dim,
                              const int64_t *const *src_per_type,
                              const int64_t *const *dst_per_type /* nullable */,
                              const int64_t *edges_per_type, const float *const *w_per_type,
                              int32_t num_types, int32_t msg_dim, int act, float *msg,
                              int64_t ld_msg, void *stream);

/* The same launch with per-edge FEATURE rows behind the gathered halves (layers built with
 * `edge_feature_dimension` / `features_dimension`): gatedmessagepassing.py:57-61
 * `edge_transformation_layer(cat([edge_source_states, features], -1))`, mlpmessagepassing.py:90-98
 * `cat([message_input, features], -1)`, the features coming from graphneuralnetwork.py:162-186:
 *   msg[off_t + e, :] = act( [ x[src_t[e]] ; x[dst_t[e]] (if dst) ; feat_t[e, :feat_dim] ] W_t^T )
 * without materialising the [E, state_dim (+ state_dim) + feat_dim] input matrix.
 *   feat_per_type: HOST array of device pointers, feat_t = [E_t, feat_dim] with row stride ld_feat;
 *   w_per_type[t]: [msg_dim, state_dim * (dst ? 2 : 1) + feat_dim] row-major contiguous.
 * Requires feat_dim > 0, feat_dim % 4 == 0, ld_feat % 4 == 0 and 16-byte aligned feature rows (callers zero-pad odd
 * widths, and the weight columns with them: the padded products are exact zeros) next to the requirements above. */
int ptgnn_amd_edge_linear_feat_f32(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                   const int64_t *const *src_per_type,
                                   const int64_t *const *dst_per_type /* nullable */,
                                   const float *const *feat_per_type, int64_t ld_feat, int32_t feat_dim,
                                   const int64_t *edges_per_type, const float *const *w_per_type,
                                   int32_t num_types, int32_t msg_dim, int act, float *msg,
                                   int64_t ld_msg, void *stream);

/* ------------------------------------------------------------------------------------------
 * Training variants of the per-edge message GEMM (GGNN, gatedmessagepassing.py:57-61:
 * `edge_transformation_layer(self.__dropout(cat([edge_source_states, features])))`).
 *
 * ptgnn_amd_edge_linear_dropout_f32: as ptgnn_amd_edge_linear_f32 (no target-state half, no
 * activation) with nn.Dropout(p) folded in.  The keep mask is a counter-based hash of
 * (dropout_seed, global message row, forward input column) -- see ptgnn_amd/csrc/dense_common.h --
 * so no [E, H] mask tensor exists and the backward kernels regenerate it:
 *   dropout_mode 1: mask the gathered INPUT rows        msg = (mask * x[src] / (1-p)) W_t^T   (forward)
 *   dropout_mode 2: mask the OUTPUT rows                out = (x[src] W_t^T) * mask / (1-p)
 *                   (backward w.r.t. the gathered input: x = d_msg, src = identity index,
 *                    w_per_type = W_t^T [state_dim_fwd, msg_dim_fwd]; here msg_dim = forward state_dim)
 *   dropout_mode 0 or dropout_p == 0: plain ptgnn_amd_edge_linear_f32.
 * The mask is Bernoulli(1 - p') per element with p' = round(p * 65536) / 65536.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_edge_linear_dropout_f32(const float *x, int64_t ld_x,
        int64_t num_rows /* rows of x: gathered node ids are clamped into [0, num_rows) */,
        int32_t state_dim,
                                      const int64_t *const *src_per_type,
                                      const int64_t *edges_per_type, const float *const *w_per_type,
                                      int32_t num_types, int32_t msg_dim, float *msg, int64_t ld_msg,
                                      int dropout_mode, float dropout_p, uint64_t dropout_seed,
                                      void *stream);

/* ------------------------------------------------------------------------------------------
 * The same per-edge dropout with the keep mask as ONE BIT per element (round 4).  Evaluating the hash
 * inside the forward, input-gradient and weight-gradient GEMMs costs ~55 vector instructions per 16
 * MFMAs, and on gfx950 fp32 MFMA shares the vector lanes with the VALU; as bits the mask costs one
 * dword load per 32 columns and 3-4 instructions per element.
 *
 * ptgnn_amd_dropout_bitmask: bits[row * (width / 32) + c], bit b = keep flag of column 32 c + b of message
 *   row `row`, from the SAME hash of (dropout_seed, row, column) the *_dropout_f32 / *_weight_grad_f32
 *   entry points evaluate -- the two families are interchangeable and bit-identical.  width % 32 == 0;
 *   `bits` holds ptgnn_amd_dropout_bitmask_bytes(rows, width) bytes.  One mask serves the forward, the
 *   input gradient and the weight gradient of one layer call (E * H / 8 bytes; the gathered [E, H] input
 *   it replaces is 32 x that).
 * ptgnn_amd_edge_linear_masked_f32: ptgnn_amd_edge_linear_dropout_f32 (modes 1 and 2, same argument
 *   meaning) with `mask_bits` in place of the seed; runs on the fence-free streaming kernel.  Shapes:
 *   ptgnn_amd_edge_linear_masked_supported(state_dim, msg_dim, mode) (state_dim in {64, 128, 256},
 *   msg_dim in {64, 128, 256}); anything else returns EUNSUPPORTED -- use the *_dropout_f32 form there.
 * ptgnn_amd_edge_weight_grad_masked_f32: ptgnn_amd_edge_weight_grad_f32 (no target-state half) with
 *   `mask_bits`; shapes: ptgnn_amd_edge_weight_grad_masked_supported (state_dim % 128 == 0, msg_dim % 32 == 0).
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_dropout_bitmask_bytes(int64_t rows, int32_t width);
int ptgnn_amd_dropout_bitmask(int64_t rows, int32_t width, float dropout_p, uint64_t dropout_seed,
                              uint32_t *bits, void *stream);
int ptgnn_amd_edge_linear_masked_supported(int32_t state_dim, int32_t msg_dim, int dropout_mode);
int ptgnn_amd_edge_linear_masked_f32(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                     const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                     const float *const *w_per_type, int32_t num_types, int32_t msg_dim,
                                     float *msg, int64_t ld_msg, int dropout_mode, float dropout_p,
                                     const uint32_t *mask_bits, void *stream);
int ptgnn_amd_edge_weight_grad_masked_supported(int32_t state_dim, int32_t msg_dim);
int ptgnn_amd_edge_weight_grad_masked_f32(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                          const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                          const float *grad_msg, int64_t ld_grad_msg, int32_t num_types,
                                          int32_t msg_dim, float dropout_p, const uint32_t *mask_bits,
                                          float *grad_w, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weight gradient of the per-edge message Linear for every edge type in one call (autograd of the
 * nn.Linear at gatedmessagepassing.py:20-23,57-61 / the MLP output layer at mlpmessagepassing.py:96-98):
 *   grad_w[t, m, k] = sum_{e < E_t} grad_msg[off_t + e, m] * in_t[e, k],
 *   in_t[e, :] = [ x[src_t[e], :] ; x[dst_t[e], :] (if dst_per_type) ]  (* dropout mask if dropout_p > 0)
 *   grad_w: [num_types, msg_dim, in_dim] contiguous, in_dim = state_dim * (dst ? 2 : 1); types without
 *           edges get zeros.  Deterministic: chunk partials on fp32 MFMA, then an ordered reduction.
 *   workspace: ptgnn_amd_edge_wgrad_workspace_bytes(total edges, num_types, msg_dim, in_dim) bytes.
 * Requires state_dim % 4 == 0, msg_dim % 4 == 0, 16-byte aligned rows (else EUNSUPPORTED).
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_edge_wgrad_workspace_bytes(int64_t num_edges, int32_t num_types, int32_t msg_dim,
                                            int32_t in_dim);
int ptgnn_amd_edge_weight_grad_f32(const float *x, int64_t ld_x,
        int64_t num_rows /* rows of x: gathered node ids are clamped into [0, num_rows) */,
        int32_t state_dim,
                                   const int64_t *const *src_per_type,
                                   const int64_t *const *dst_per_type /* nullable */,
                                   const int64_t *edges_per_type, const float *grad_msg,
                                   int64_t ld_grad_msg, int32_t num_types, int32_t msg_dim,
                                   float dropout_p, uint64_t dropout_seed, float *grad_w,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* Dense form: grad_w [n_out, k] = grad_y^T . x over `rows` rows, and (grad_b non-null) the bias
 * gradient grad_b [n_out] = column sums of grad_y from the same pass (autograd of nn.Linear /
 * nn.GRUCell parameters, gatedmessagepassing.py:25, mlpmessagepassing.py:60-63).  Workspace:
 * ptgnn_amd_edge_wgrad_workspace_bytes(rows, 1, n_out, k). */
int ptgnn_amd_linear_weight_grad_f32(const float *x, int64_t ld_x, int32_t k, const float *grad_y,
                                     int64_t ld_grad_y, int64_t rows, int32_t n_out, float *grad_w,
                                     float *grad_b /* nullable */, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Training form of the fused GRU cell (autograd of nn.GRUCell, gatedmessagepassing.py:25,69).
 * ptgnn_amd_gru_cell_train_f32: as ptgnn_amd_gru_cell_f32, additionally writes
 *   gates [n, 4*hd] = [ r | z | n | gh_n ]  (gh_n = W_hn h + b_hn) for the backward.
 * ptgnn_amd_gru_cell_backward_gates_f32: the gate math's backward,
 *   d_gi [n, 3hd], d_gh [n, 3hd] (gradients of the two gate pre-activations, gate order r, z, n) and
 *   d_h [n, hd] = grad_out * z (the direct path); the GEMM halves follow with ptgnn_amd_linear_f32 /
 *   ptgnn_amd_linear_weight_grad_f32.  Requires hd % 4 == 0 and 16-byte aligned rows.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_gru_cell_train_f32(const float *a, int64_t ld_a, const float *h, int64_t ld_h,
                                 const float *w_ih, const float *w_hh, const float *b_ih,
                                 const float *b_hh, int64_t n, int32_t m, int32_t hd, float *out,
                                 int64_t ld_out, float *gates, void *stream);
int ptgnn_amd_gru_cell_backward_gates_f32(const float *grad_out, int64_t ld_grad_out, const float *gates,
                                          const float *h, int64_t ld_h, int64_t n, int32_t hd,
                                          float *d_gi, float *d_gh, float *d_h, void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the segment reduce w.r.t. the message matrix (the autograd torch_scatter supplies
 * behind abstractmessagepassing.py:44-50):
 *   out[perm[s], :] = grad[slot_row[s], :]                                   sum / mean (pre-scaled)
 *   out[perm[s], c] = arg[slot_row[s], c] == s ? grad[slot_row[s], c] : 0    max / min
 *   slot_row int32 [num_slots]: destination row of CSR slot s (rowptr expanded); arg: the argout of
 *   ptgnn_amd_gather_reduce_f32 ([num_rows, dim], nullable); out [num_slots, dim] message order.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_segment_spread_f32(const float *grad, int64_t ld_grad, const int32_t *arg /* nullable */,
                                 const int32_t *slot_row, const int32_t *perm, int64_t num_slots,
                                 int32_t dim, float *out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Row epilogue of the MLP message-passing layer as a differentiable pair (the training step; in inference the
 * same arithmetic is the `epilogue` of ptgnn_amd_gather_reduce_f32):
 *   y = LayerNorm(GELU(x))   with `flags` = PTGNN_AMD_EPI_* naming which of the two apply
 * Replaces: nn.GELU() -> nn.LayerNorm(message_dimension) at mlpmessagepassing.py:20,44-47,114-116 and their autograd
 *   (exact-erf GELU; LayerNorm eps / affine as given; two-pass mean / variance), x, y, grad_* [rows, dim] fp32,
 *   dim <= 512.  The forward equals the fused inference epilogue bit for bit.
 * Backward: grad_x [rows, dim]; grad_gamma / grad_beta [dim] (LayerNorm only; OVERWRITTEN, deterministic: per-
 *   workgroup partial rows in `workspace` (ptgnn_amd_row_epilogue_workspace_bytes) summed in a fixed order).
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_row_epilogue_f32(const float *x, int64_t ld_x, int64_t rows, int32_t dim, int32_t flags,
                               const float *ln_gamma /* nullable without LayerNorm */,
                               const float *ln_beta /* nullable without LayerNorm */, float ln_eps, float *y,
                               int64_t ld_y, void *stream);
size_t ptgnn_amd_row_epilogue_workspace_bytes(int64_t rows, int32_t dim);

/* Backward of the node update's activation + dropout (mlpmessagepassing.py:62-66: Linear -> Tanh -> Dropout) in one
 * pass: out[i] = grad[i] * (keep[i] ? scale : 0) * act'(y[i]) with y = the activation's OUTPUT (tanh': 1 - y^2,
 * relu': y > 0, none: 1), keep = the dropout's boolean mask (one byte per element; NULL = no dropout), scale = 1/(1-p).
 * Contiguous arrays of n elements (any n: the n % 4 tail runs on one scalar lane), 16-byte aligned (else EUNSUPPORTED). */
int ptgnn_amd_act_dropout_backward_f32(const float *grad, const float *y, const uint8_t *keep, float scale, int act,
                                       int64_t n, float *out, void *stream);
int ptgnn_amd_row_epilogue_backward_f32(const float *x, int64_t ld_x, const float *grad_y, int64_t ld_gy,
                                        int64_t rows, int32_t dim, int32_t flags, const float *ln_gamma,
                                        float ln_eps, float *grad_x, int64_t ld_gx,
                                        float *grad_gamma /* nullable without LayerNorm */,
                                        float *grad_beta /* nullable without LayerNorm */, void *workspace,
                                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * h' = GRUCell(a, h)  (gate order r, z, n), gatedmessagepassing.py:25,69.
 *   a [n, m], h [n, hd], w_ih [3hd, m], w_hh [3hd, hd], b_ih/b_hh [3hd], out [n, hd].
 *   Gate GEMMs run on fp32 MFMA with the gate non-linearities fused in the epilogue; no
 *   [n, 3hd] intermediates reach HBM.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_gru_cell_f32(const float *a, int64_t ld_a, const float *h, int64_t ld_h,
                           const float *w_ih, const float *w_hh, const float *b_ih,
                           const float *b_hh, int64_t n, int32_t m, int32_t hd, float *out,
                           int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weighted-sum pooling of elements into samples (nodes into graphs):
 *   out[g, :] = sum_{i : map[i] == g} sigmoid(x[i, :] . w) * x[i, :]
 * Replaces: WeightedSumVarSizedElementReduce.forward, ptgnn/neuralmodels/reduceops/varsizedsummary.py:68-81 --
 *   nn.Linear(D, 1, bias=False) (a gemv), torch.sigmoid, the broadcast multiply that materialises [N, D] and
 *   torch_scatter.scatter_sum -- as used by GruGlobalStateUpdate (globalgraphexchange.py:37-45) in the VarMisuse GGNN
 *   stack (varmisuse/train.py:87-92).  One pass over x; no float atomics: a segment is cut into 128-row chunks counted
 *   from its own start, the chunk partials are added in chunk order -- a fixed function of the segment's rows and their
 *   order, wherever the segment sits in the batch (not the reference's serial fold order: fp32 rounding only).
 *   x [num_elements, dim], w [dim], rowptr int32 [num_segments + 1] / perm int32 [num_elements]: the stable plan of the
 *   element -> sample map (ptgnn_amd_csr_build over (map, map); perm[s] = element of plan slot s), out [num_segments, dim].
 *   dim <= 1024.  workspace: ptgnn_amd_weighted_pool_workspace_bytes.
 * Backward: grad_x [num_elements, dim] and grad_w [dim] (both OVERWRITTEN; grad_w deterministic) from
 *   grad_out [num_segments, dim] and the int64 map itself.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_weighted_pool_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim);
int ptgnn_amd_weighted_pool_f32(const float *x, int64_t ld_x, const float *w, const int32_t *rowptr,
                                const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim,
                                float *out, int64_t ld_out, void *workspace, size_t workspace_bytes, void *stream);
size_t ptgnn_amd_weighted_pool_backward_workspace_bytes(int64_t num_elements, int32_t dim);
int ptgnn_amd_weighted_pool_backward_f32(const float *x, int64_t ld_x, const float *w, const int64_t *map,
                                         const float *grad_out, int64_t ld_go, int64_t num_elements, int32_t dim,
                                         float *grad_x, int64_t ld_gx, float *grad_w, void *workspace,
                                         size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Attention pooling of elements into samples, `heads` softmax heads over the same element rows:
 *   s[i,h] = u[g,h,:] . x[i,:]  (g = map[i]),   p[i,h] = exp(s[i,h] - lse[g,h]),   out[g,h,:] = sum_{i : map[i] == g} p[i,h] x[i,:]
 * Replaces: SelfAttentionVarSizedElementReduce.forward and MultiheadSelfAttentionVarSizedElementReduce.forward,
 *   ptgnn/neuralmodels/reduceops/varsizedsummary.py:99-113 and :140-178 -- `queries[map]`, the key `nn.Linear` over all
 *   elements, the einsum, `exp(scatter_log_softmax(eps=0))`, the broadcast multiply that materialises [N, heads * D] and
 *   `scatter_sum` -- as used by the Graph2Seq summariser (graph2seq/graph2seq.py:56-66,116-122).  The key Linear moves
 *   onto the samples: u = c * blockdiag(q) W_k (ptgnn_amd_head_projection_f32, mode 0), c = 1 / sqrt(hidden / heads)
 *   for the multi-head class and 1 for the single-head one.  One pass over x: online softmax per 128-row chunk counted
 *   from the sample's own start, chunks merged in chunk order (no float atomics; deterministic).
 *   x [num_elements, dim] (ld_x), u [num_segments, heads, dim] contiguous, rowptr / perm: the stable plan of the map
 *   (as ptgnn_amd_weighted_pool_f32), out [num_segments, heads, dim] contiguous, stats [num_segments, 2 * heads]: per
 *   (g, h) the max score and the log-sum-exp (0 for a sample without elements, whose out rows are 0).
 *   1 <= heads <= 8 and dim <= 1024 (ptgnn_amd_attention_pool_supported), else EUNSUPPORTED.
 *   workspace: ptgnn_amd_attention_pool_workspace_bytes.
 * Backward (one pass over x): from grad_out = dL/dout [num_segments, heads, dim] and the forward's out and stats,
 *   grad_x [num_elements, dim] (ld_gx; every element of the plan OVERWRITTEN) and grad_u [num_segments, heads, dim]
 *   (deterministic: chunk partials folded in chunk order).  workspace: ptgnn_amd_attention_pool_backward_workspace_bytes.
 * ptgnn_amd_head_projection_f32: the per-head block products around the pool, on [rows, ...] tensors (dk = head_dim,
 *   hidden = heads * dk, w [hidden, dim], all contiguous):
 *   mode 0  out[g,h,:] = scale * w[h*dk:(h+1)*dk, :]^T a[g, h*dk:(h+1)*dk]   a [rows, hidden] -> out [rows, heads, dim]
 *           (the key projection of the queries; the input gradient of mode 1)
 *   mode 1  out[g, j]  = scale * w[j, :] . b[g, j / dk, :]                    b [rows, heads, dim] -> out [rows, hidden]
 *           (the value Linear on the pools, varsizedsummary.py:161-166; the input gradient of mode 0)
 *   mode 2  out[j, :]  = scale * sum_g a[g, j] b[g, j / dk, :]                 -> out [hidden, dim], a fixed order
 *           (the weight gradient of modes 0 and 1)
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_attention_pool_supported(int32_t dim, int32_t num_heads);
size_t ptgnn_amd_attention_pool_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                int32_t num_heads);
int ptgnn_amd_attention_pool_f32(const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                                 const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim,
                                 int32_t num_heads, float *out, float *stats, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t ptgnn_amd_attention_pool_backward_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                         int32_t num_heads);
int ptgnn_amd_attention_pool_backward_f32(const float *x, int64_t ld_x, const float *u, const int32_t *rowptr,
                                          const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim,
                                          int32_t num_heads, const float *out, const float *stats,
                                          const float *grad_out, float *grad_x, int64_t ld_gx, float *grad_u,
                                          void *workspace, size_t workspace_bytes, void *stream);
int ptgnn_amd_head_projection_f32(int mode, const float *a /* nullable in mode 1 */,
                                  const float *b /* nullable in mode 0 */, const float *w /* nullable in mode 2 */,
                                  int64_t num_rows, int32_t num_heads, int32_t head_dim, int32_t dim, float scale,
                                  float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scores of elements against the `vectors` of their sample, and their per-sample log-sum-exp:
 *   scores[i,l] = v[g,l,:] . y[i,:]  (g = map[i]),   lse[g,l] = log sum_{i : map[i] == g} exp(scores[i,l])
 * Replaces: the copy attention of GruCopyingDecoder._compute_logprobs, ptgnn/neuralmodels/sequence/grucopydecoder.py:
 *   the gather `output_states[input_memories_origin_idx]` that materialises [num_inputs, L, H] (:89-91), the einsum
 *   "ilh,ih->il" (:95-97) and `scatter_logsumexp(copy_attention_scores, ..., eps=0)` (:122-124).  With dropout active the
 *   rows y are dropout(memories_to_copy_attention(input_memories)) (:83-86) and v the GRU's output states; without it
 *   the Linear moves onto the samples (v = W_c^T o) and y are the memories themselves.  One pass over y: running
 *   (max, sum) per 128-row chunk counted from the sample's own start, chunks merged in chunk order (no float atomics;
 *   a sample's lse has the same bits alone and inside a batch).
 *   y [num_elements, dim] (ld_y), v [num_segments, vectors, dim] contiguous, rowptr / perm: the stable plan of the map
 *   (as ptgnn_amd_weighted_pool_f32), scores [num_elements, vectors] contiguous in ELEMENT order, lse [num_segments,
 *   vectors] (-inf for a sample without elements).
 *   1 <= vectors <= 8 and dim <= 1024 (ptgnn_amd_segment_scores_supported), else EUNSUPPORTED.
 *   workspace: ptgnn_amd_segment_scores_workspace_bytes.
 * Backward (one pass over y; replaces the autograd of :89-97,122-124): from grad_scores [num_elements, vectors],
 *   grad_lse [num_segments, vectors] and the forward's scores and lse,
 *   t[i,l] = grad_scores[i,l] + grad_lse[g,l] exp(scores[i,l] - lse[g,l]),
 *   grad_y[i,:] = sum_l t[i,l] v[g,l,:] (ld_gy; every element of the plan OVERWRITTEN) and
 *   grad_v[g,l,:] = sum_{i in g} t[i,l] y[i,:] (deterministic: chunk partials folded in chunk order; 0 for a sample
 *   without elements).  workspace: ptgnn_amd_segment_scores_backward_workspace_bytes.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_segment_scores_supported(int32_t dim, int32_t num_vectors);
size_t ptgnn_amd_segment_scores_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                int32_t num_vectors);
int ptgnn_amd_segment_scores_f32(const float *y, int64_t ld_y, const float *v, const int32_t *rowptr,
                                 const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim,
                                 int32_t num_vectors, float *scores, float *lse, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t ptgnn_amd_segment_scores_backward_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim,
                                                         int32_t num_vectors);
int ptgnn_amd_segment_scores_backward_f32(const float *y, int64_t ld_y, const float *v, const int32_t *rowptr,
                                          const int32_t *perm, int64_t num_segments, int64_t num_elements, int32_t dim,
                                          int32_t num_vectors, const float *scores, const float *lse,
                                          const float *grad_scores, const float *grad_lse, float *grad_y, int64_t ld_gy,
                                          float *grad_v, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * GraphNorm: per-graph normalisation of node states, per graph g with n_g nodes, per column, fp32:
 *   mu[g] = (1/n_g) sum_{i in g} x_i      s_i = x_i - alpha * mu[g]      sig2[g] = (1/n_g) sum_{i in g} s_i^2 + eps
 *   y_i = gamma * s_i / sqrt(sig2[g]) + bias
 * Replaces: GraphNorm.forward, ptgnn/neuralmodels/gnn/messagepassing/graphnorm.py:36-46 -- two torch_scatter.scatter_mean
 *   calls, the gathers mean[idx] and sigma_2[idx] and the elementwise pow / sub / mul / sqrt / div / add, each of which
 *   materialises [N, D].  Three reads of x and one write of y; no float atomics: a graph is cut into 128-row chunks
 *   counted from its own start, the chunk partials are added in chunk order -- a graph's statistics and output rows are a
 *   fixed function of its rows and their order, wherever the graph sits in the batch.  sig2 is the two-pass variance over
 *   the rounded s_i (alpha * mu rounded, then the subtraction rounded), as the reference's.
 *   x [num_elements, dim] (ld_x), gamma / alpha / bias [dim], rowptr int32 [num_segments + 1] / perm int32 [num_elements]:
 *   the stable plan of the node -> graph map (any map; as ptgnn_amd_weighted_pool_f32), y [num_elements, dim] (ld_y):
 *   every row named by perm OVERWRITTEN.  mean (nullable: inference) [num_segments, dim]: mu per graph (0 for a graph
 *   without nodes), all the backward needs from the forward.  dim <= 1024 (ptgnn_amd_graph_norm_supported), else
 *   EUNSUPPORTED.  workspace: ptgnn_amd_graph_norm_workspace_bytes.
 * Backward: with r = 1/sqrt(sig2), gy = grad_y [num_elements, dim] (ld_gy), A = sum gy_i, B = sum gy_i s_i, C = sum s_i,
 *   c = -gamma B r^3 / n_g, S = gamma r A + c C.  s_i is re-formed from the forward's `mean` (the same rounded s_i); A, B, C
 *   and sum s_i^2 are summed with float64 accumulators and sig2 (from `eps`, the forward's), r, c, S formed in float64:
 *   S cancels to ~0 on one- and two-node graphs, which fp32 per-graph arithmetic does not survive.
 *   grad_x_i = gamma r gy_i + c s_i - (alpha / n_g) S    [num_elements, dim] (ld_gx), every row named by perm,
 *   grad_gamma = sum_g B r,  grad_alpha = -sum_g mu S,  grad_bias = sum_g A   [dim] each, graphs added in graph order.
 *   Two reads of (x, grad_y), one write of grad_x.  All outputs OVERWRITTEN and deterministic.
 *   workspace: ptgnn_amd_graph_norm_backward_workspace_bytes.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_graph_norm_supported(int32_t dim);
size_t ptgnn_amd_graph_norm_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim);
int ptgnn_amd_graph_norm_f32(const float *x, int64_t ld_x, const float *gamma, const float *alpha, const float *bias,
                             float eps, const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                             int64_t num_elements, int32_t dim, float *y, int64_t ld_y, float *mean /* nullable */,
                             void *workspace, size_t workspace_bytes, void *stream);
size_t ptgnn_amd_graph_norm_backward_workspace_bytes(int64_t num_segments, int64_t num_elements, int32_t dim);
int ptgnn_amd_graph_norm_backward_f32(const float *x, int64_t ld_x, const float *grad_y, int64_t ld_gy,
                                      const float *gamma, const float *alpha, float eps, const float *mean,
                                      const int32_t *rowptr, const int32_t *perm, int64_t num_segments,
                                      int64_t num_elements, int32_t dim,
                                      float *grad_x, int64_t ld_gx, float *grad_gamma, float *grad_alpha,
                                      float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Block self-attention among the nodes of each window of a graph, the core of MultiHeadSelfAttentionMessagePassing.
 * Windows (ptgnn_amd_attention_windows).  Replaces: __iter_idxs_per_graph,
 *   ptgnn/neuralmodels/gnn/messagepassing/selfattmessagepassing.py:59-75 -- scatter_sum of ones, then a Python loop that
 *   yields torch.arange per window.  Graph g owns the rows rowptr[g] .. rowptr[g + 1] - 1 (rowptr int32
 *   [num_graphs + 1]: the prefix sums of the per-graph node counts, i.e. the rowptr of the plan of the node -> graph map;
 *   only the COUNTS of the map matter, as in the reference) and is cut every max_num_nodes rows; a graph without nodes
 *   gives no window.  windows int32 [capacity], capacity >= ptgnn_amd_attention_windows_bound(...) + 1 =
 *   ceil(num_rows / max_num_nodes) + num_graphs + 1: windows[w] = first row of window w for the W windows of the batch,
 *   windows[W .. bound] = num_rows (window w is rows windows[w] .. windows[w + 1] - 1; the ones past W are empty).  One
 *   launch, no host read-back.
 * Attention (ptgnn_amd_block_attention_f32).  Replaces: selfattmessagepassing.py:104-117 -- per window the gathers
 *   keys[graph_nodes] / queries[...] / values[...], einsum("khd,vhd->khv") / sqrt(dk), softmax over v, dropout,
 *   einsum("khv,vhd->khd"), and the torch.cat of the windows.  Per window and head, exact fp32 (fp32 MFMA):
 *     S[k, v] = key_k . query_v / sqrt(dk)    P = dropout(softmax_v(S))    out_k = sum_v P[k, v] value_v
 *   (the row side is the key, the softmax runs over the queries: the reference's order).  kqv [num_rows, heads (2 dk + dv)]
 *   (ld_kqv) is read in place, per head [keys dk | queries dk | values dv]; `windows` / num_windows: the table above and
 *   its bound (num_windows + 1 entries are read; no window may be longer than max_num_nodes).  Flash-style: a window is
 *   walked in 32-row tiles through LDS with a running max and sum, the [n, n] scores are never written.
 *   out [num_rows, heads dv] (ld_out) and lse [num_rows, heads] (the log-sum-exp of every score row, which the backward
 *   takes) are OVERWRITTEN for every row inside a window.  dropout_p in [0, 1): 0 = off; otherwise element (row r, head
 *   h, window column j) is multiplied by the stateless hash mask of row r heads + h, column j of a [num_rows heads, W]
 *   mask, W = max_num_nodes rounded up to even (tests/helpers.py dropout_keep_scale), after the normalisation.
 *   1 <= dk, dv <= 128 (ptgnn_amd_block_attention_supported), else EUNSUPPORTED.
 * Backward (ptgnn_amd_block_attention_backward_f32): autograd of lines 104-117.  P = exp(S - lse) is recomputed,
 *   D_k = sum_d grad_out[k, d] out[k, d], dS = P o (M o dP - D), dP[k, v] = grad_out_k . value_v (M: the forward's mask):
 *     grad key_k = sum_v dS[k, v] query_v / sqrt(dk)   grad query_v = sum_k dS[k, v] key_k / sqrt(dk)
 *     grad value_v = sum_k (M o P)[k, v] grad_out_k
 *   written into grad_kqv [num_rows, heads (2 dk + dv)] (ld_gkqv) in the layout of kqv, every row inside a window
 *   OVERWRITTEN.  Every sum runs in tile order inside one wave: no float atomics, deterministic, and a window's rows do
 *   not depend on its place in the batch.  workspace: ptgnn_amd_block_attention_backward_workspace_bytes (D).
 * Bad arguments are refused before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_block_attention_supported(int32_t dk, int32_t dv);
int64_t ptgnn_amd_attention_windows_bound(int64_t num_graphs, int64_t num_rows, int32_t max_num_nodes);
int ptgnn_amd_attention_windows(const int32_t *rowptr, int64_t num_graphs, int64_t num_rows, int32_t max_num_nodes,
                                int32_t *windows, int64_t capacity, void *stream);
int ptgnn_amd_block_attention_f32(const float *kqv, int64_t ld_kqv, const int32_t *windows, int64_t num_windows,
                                  int64_t num_rows, int32_t max_num_nodes, int32_t num_heads, int32_t dk, int32_t dv,
                                  float dropout_p, uint64_t seed, float *out, int64_t ld_out, float *lse, void *stream);
size_t ptgnn_amd_block_attention_backward_workspace_bytes(int64_t num_rows, int32_t num_heads);
int ptgnn_amd_block_attention_backward_f32(const float *kqv, int64_t ld_kqv, const float *out, int64_t ld_out,
                                           const float *lse, const float *grad_out, int64_t ld_go,
                                           const int32_t *windows, int64_t num_windows, int64_t num_rows,
                                           int32_t max_num_nodes, int32_t num_heads, int32_t dk, int32_t dv,
                                           float dropout_p, uint64_t seed, float *grad_kqv, int64_t ld_gkqv,
                                           void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * EGC-S layer (egcmessagepassing.py:63-91; aggregation abstractmessagepassing.py:38-50), K heads, B bases,
 * Dh = D / K, message rows [K, B, Dh] (msg_dim = K*B*Dh):
 *   out[v, k*Dh + d] = sum_b coef[v, k*B + b] * agg[v, k*B*Dh + b*Dh + d],   agg = reduce over the in-edges of v.
 *
 * ptgnn_amd_egc_gather_combine_f32: the aggregation of ptgnn_amd_gather_reduce_f32 (same plan, `msg`/`col`/`type_bits`
 *   table or edge forms, hub rows and workspaces; no destination term, no epilogue) with the combine as its row finish:
 *   the [N, msg_dim] aggregate is not written unless `agg_out` (nullable, [N, msg_dim] contiguous) is given; `argout`
 *   (nullable, max/min only, needs agg_out) as in ptgnn_amd_gather_reduce_f32.  coef [N, K*B] (ld_coef), out [N, K*Dh]
 *   (ld_out).  PTGNN_AMD_EUNSUPPORTED when msg_dim exceeds one lane group's row (512 on 16-byte aligned float rows,
 *   256 otherwise): the caller then aggregates with ptgnn_amd_gather_reduce_f32 and combines separately.
 * ptgnn_amd_egc_combine_f32: the combine alone, agg [rows, K*B*Dh] (ld_agg) -> out [rows, K*Dh]; any K, B, Dh.
 * ptgnn_amd_egc_combine_backward_f32: from grad = dL/dout [rows, K*Dh], in one pass (both outputs OVERWRITTEN)
 *   grad_agg[v, k,b,d] = coef[v, k*B + b] * grad[v, k*Dh + d]     grad_coef[v, k*B + b] = sum_d agg[v, k,b,d] * grad[v, k*Dh + d].
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_egc_gather_combine_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr, const int32_t *col,
                                     int32_t type_bits, int64_t num_nodes, int32_t num_heads, int32_t num_bases,
                                     int32_t head_dim, int reduce, const float *coef, int64_t ld_coef, float *out,
                                     int64_t ld_out, float *agg_out /* nullable */, int32_t *argout /* nullable */,
                                     int64_t num_edges, int32_t hub_threshold,
                                     const int32_t *hub_entries /* nullable */, const int32_t *hub_count /* nullable */,
                                     void *hub_ws /* nullable */, size_t hub_ws_bytes,
                                     int32_t *hub_tickets /* nullable */, void *stream);
int ptgnn_amd_egc_combine_f32(const float *agg, int64_t ld_agg, const float *coef, int64_t ld_coef, int64_t num_rows,
                              int32_t num_heads, int32_t num_bases, int32_t head_dim, float *out, int64_t ld_out,
                              void *stream);
int ptgnn_amd_egc_combine_backward_f32(const float *agg, int64_t ld_agg, const float *coef, int64_t ld_coef,
                                       const float *grad, int64_t ld_grad, int64_t num_rows, int32_t num_heads,
                                       int32_t num_bases, int32_t head_dim, float *grad_agg, int64_t ld_grad_agg,
                                       float *grad_coef, int64_t ld_grad_coef, void *stream);

/* ------------------------------------------------------------------------------------------
 * PNA aggregation (pna_aggregation.py:27-56, PnaMessageAggregation(delta)) over a plan of ptgnn_amd_csr_build.  Per
 * destination row v with in-degree d (its CSR slots) and message rows m_e:
 *   A   = [sum, mean, max, min, std]   (5 blocks of msg_dim columns, fp32)
 *         sum = sum_e m_e (slot order)      mean = sum / (float(d) + 1e-5)
 *         max / min as ptgnn_amd_gather_reduce_f32 (0 for empty rows, ties -> the earliest slot)
 *         std = sqrt(sum_e (relu(m_e*m_e - mean*mean) + 1e-10)), m*m and mean*mean each rounded (no contraction)
 *   s   = log(float(d) + 1) / delta,  s' = 1 / (s + 1e-3)
 *   out = [A | A*s | A*s']             ([N, 15*msg_dim], ld_out)
 * then, with `epilogue` (PTGNN_AMD_EPI_*), GELU (erf form) and / or an affine LayerNorm over the 15*msg_dim columns
 * (ln_gamma / ln_beta [15*msg_dim], ln_eps) -- msg_dim <= 256 only (else EUNSUPPORTED).
 * Messages: `ysrc` / `ydst` / `col` / `type_bits` as in ptgnn_amd_gather_reduce_f32 (table form with an optional
 *   destination term; edge form: [E, msg_dim] messages with col = the plan's perm and type_bits = 0).
 * round_mode: 0, or 1 / 2 to round A to fp16 / bf16 before the scalers (the reference's `.to(msg_dtype)` for half /
 *   bfloat16 messages; the scaled blocks are products of the rounded values).
 * argmax / argmin: nullable together, [N, msg_dim] int32 contiguous: the winning CSR slot (-1 for empty rows); not with
 *   a destination term.
 * agg_out: nullable, [N, 5*msg_dim] contiguous: A before the rounding of round_mode (what the backward needs); not with
 *   an epilogue.
 * Rows of more than 256 in-edges are reduced by a whole workgroup (slots interleaved over its lane groups, partials
 *   combined in a fixed order): deterministic, sums in a different rounding order than the serial fold.
 *
 * ptgnn_amd_pna_aggregate_backward_f32 (edge form): from grad = dL/dout [N, 15*msg_dim] and the forward's UNROUNDED A
 *   (`agg`, ld_agg >= 5*msg_dim: only blocks 0 (sum) and 1 (mean) are read; std is recomputed) and args, for every
 *   slot i of row v
 *   writes row col[i] of grad_msg ([E, msg_dim], ld_grad_msg; every row referenced by `col` is OVERWRITTEN):
 *     g_k = grad[v, k] + s*grad[v, 5+k] + s'*grad[v, 10+k]   (block k of A),  gS = g_4 / (2*std),
 *     P   = #{slots of v with m*m - mean*mean > 0}  (per column),
 *     g_m = g_0 + (g_1 - gS*2*mean*P) / (d + 1e-5) + [pos]*gS*2*m + g_2*[argmax == i] + g_3*[argmin == i]
 *   with pos = (m*m - mean*mean > 0) in the forward's fp32 arithmetic; mean, std and the std terms are formed in float64
 *   from A's sum block (they cancel to ~1e-2 of their size on degree-1 rows).  round_mode as in the forward: with 1 / 2
 *   g_k is rounded to fp16 / bf16 as the reference's autograd accumulates it, h(h(h(grad[k]) + h(s'*grad[10+k])) +
 *   h(s*grad[5+k])).
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_pna_aggregate_f32(const float *ysrc, int64_t ld_y, const float *ydst /* nullable */, int64_t ld_yd,
                                const int32_t *rowptr, const int32_t *col, int32_t type_bits, int64_t num_nodes,
                                int32_t msg_dim, float delta, int epilogue, const float *ln_gamma /* nullable */,
                                const float *ln_beta /* nullable */, float ln_eps, int32_t round_mode, float *out,
                                int64_t ld_out, int32_t *argmax /* nullable */, int32_t *argmin /* nullable */,
                                float *agg_out /* nullable */, int64_t num_edges, void *stream);
int ptgnn_amd_pna_aggregate_backward_f32(const float *msg, int64_t ld_msg, const int32_t *rowptr, const int32_t *col,
                                         int64_t num_nodes, int32_t msg_dim, float delta, const float *agg,
                                         int64_t ld_agg, const int32_t *argmax, const int32_t *argmin,
                                         const float *grad, int64_t ld_grad, float *grad_msg, int64_t ld_grad_msg,
                                         int32_t round_mode, int64_t num_edges, void *stream);

/* Row gather out[i, :] = x[idx[i], :] (F.embedding at gatedmessagepassing.py:54-56,
 * mlpmessagepassing.py:88,91) for the general per-edge path (edge features / training dropout /
 * mlp_hidden_layers > 0) and for task heads (output_node_representations[node_idx_references]). */
int ptgnn_amd_gather_rows_f32(const float *x, int64_t ld_x, const int64_t *idx, int64_t n_idx,
                              int32_t dim, float *out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Subtoken pool of SubtokenUnitEmbedder (embeddings/strelementrepresentationmodel.py:67-82: nn.Embedding over the
 * [B, max_num_subtokens] ids, the length mask, the sum / mean / max over the slot axis), without the [B, S, D] tensor:
 *   slot s of bag b is LIVE iff s < lengths[b]; dead slots are never read; ids are clamped into [0, vocab)
 *   sum :  out[b] = live table rows added in slot order
 *   mean:  that sum / (float(lengths[b]) + 1e-10f)   (fp32; the GIVEN length, also when it exceeds `slots`)
 *   max :  the running maximum from -inf; arg[b, d] (nullable, int32 [B, dim] contiguous, max only) = the first slot
 *          that attains it, -1 when none does
 *   a bag without live slot: 0 (sum / mean), -inf (max) -- as the reference.
 * table [vocab, dim] (ld_table), ids int64 [num_bags, slots] contiguous, lengths int64 [num_bags], out [num_bags, dim]
 * (ld_out); mode = PTGNN_AMD_SUM / _MEAN / _MAX.  ptgnn_amd_embedding_bag_supported (pure host): dim % 4 == 0,
 * 4 <= dim <= 1024, 1 <= slots <= 32; other shapes answer PTGNN_AMD_EUNSUPPORTED before any device work.
 *
 * Backward (autograd of the nn.Embedding at :67 through the mask and the reduction; deterministic, no float atomics):
 * the bag is a one-edge-type graph, element e = b * slots + s with source b and destination ids[e].
 *   ptgnn_amd_embedding_bag_keys: src[e] = b, key[e] = the clamped id of a live slot, `vocab` for a dead one -- the
 *     adjacency pair of ptgnn_amd_csr_build (mode 0, num_nodes = vocab + 1, num_src_rows = num_bags), whose stable sort
 *     lists the elements of every vocabulary row in element order and parks the padding in row `vocab`;
 *   ptgnn_amd_embedding_bag_backward_f32: grad_table [vocab, dim] (ld_gt; OVERWRITTEN, rows nobody references exactly 0)
 *     from grad = dL/dout [num_bags, dim] over that plan's rowptr [vocab + 2] / col / perm, walking rows [0, vocab) only
 *     (padding costs no gather) with the row walk of ptgnn_amd_gather_reduce_f32 -- hub arguments as there, built with
 *     the same threshold.  mean scales the gradient rows by 1 / (float(lengths[b]) + 1e-10f) first; max routes
 *     grad[b, d] to slot arg[b, d] only (`arg` = the forward's; `perm` is read for max only).
 *     workspace: ptgnn_amd_embedding_bag_backward_workspace_bytes(num_bags, slots, dim, mode) bytes (0 for sum).
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_embedding_bag_supported(int32_t dim, int32_t slots);
int ptgnn_amd_embedding_bag_f32(const float *table, int64_t ld_table, int64_t vocab, const int64_t *ids,
                                const int64_t *lengths, int64_t num_bags, int32_t slots, int32_t dim, int mode,
                                float *out, int64_t ld_out, int32_t *arg /* nullable */, void *stream);
int ptgnn_amd_embedding_bag_keys(const int64_t *ids, const int64_t *lengths, int64_t num_bags, int32_t slots,
                                 int64_t vocab, int64_t *src, int64_t *key, void *stream);
size_t ptgnn_amd_embedding_bag_backward_workspace_bytes(int64_t num_bags, int32_t slots, int32_t dim, int mode);
int ptgnn_amd_embedding_bag_backward_f32(const float *grad, int64_t ld_grad, const int64_t *lengths,
                                         const int32_t *arg /* max only */, int64_t num_bags, int32_t slots,
                                         int64_t vocab, int32_t dim, int mode, const int32_t *rowptr,
                                         const int32_t *col, const int32_t *perm, float *grad_table, int64_t ld_gt,
                                         int32_t hub_threshold, const int32_t *hub_entries /* nullable */,
                                         const int32_t *hub_count /* nullable */, void *hub_ws /* nullable */,
                                         size_t hub_ws_bytes, int32_t *hub_tickets /* nullable */, void *workspace,
                                         size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The char-CNN of CharUnitEmbedder (embeddings/strelementrepresentationmodel.py:128-142: one_hot, three nn.Conv1d with
 * ReLU between them, max over the positions), channel-last on ROW FRAMES: every activation / gradient matrix holds
 * R = length - k1 + 1 rows per sample, sample b at rows [b R, (b + 1) R); layer i's valid positions are the first P_i
 * rows of a sample (P1 = R, P2 = R - k2 + 1, P3 = P2 - k3 + 1), the rows behind them are computed and ignored.
 *
 * ptgnn_amd_char_embed_f32 (:133-137, one_hot + transpose + float + conv_l1, and the ReLU of :138): a convolution over a
 *   one-hot input is a table sum,
 *     out[b R + p, :] = act(bias + sum_{k < window} table[k num_chars + chars[b, p + k], :]),   p < R,
 *   chars int64 [num_samples, length] contiguous, table [window num_chars, dim] contiguous with row k C + c = W1[:, c, k],
 *   bias [dim] (nullable), out [num_samples R, dim] (ld_out), act = PTGNN_AMD_ACT_NONE / _RELU.  One launch; ids outside
 *   [0, num_chars) are clamped into it.  ptgnn_amd_char_embed_supported (pure host): dim % 4 == 0, 4 <= dim <= 1024,
 *   1 <= window <= 16 and (window num_chars + 1) * 256 bytes <= 160 KiB (the backward's LDS tile); other shapes answer
 *   PTGNN_AMD_EUNSUPPORTED before any device work.
 * ptgnn_amd_char_embed_backward_f32 (autograd of :133-138 w.r.t. conv_l1's weight and bias): from grad = dL/dout
 *   [num_samples R, dim] (ld_grad) and the saved out = a1 (ld_a1; read for _RELU only: the mask a1 > 0) it OVERWRITES
 *   grad_table [window num_chars, dim] and grad_bias [dim] (nullable).  Deterministic, no float atomics: a wave owns
 *   ptgnn_amd_char_embed_backward_chunk() consecutive samples and 64 columns, adds them in row order into an LDS copy of
 *   the table tile, and the chunks' tiles are folded in chunk order.  workspace:
 *   ptgnn_amd_char_embed_backward_workspace_bytes(num_samples, num_chars, window, dim) bytes.
 *
 * ptgnn_amd_window_linear_f32 (nn.Conv1d at :138-139 on a channel-last frame, and its input gradient):
 *     y[r, :] = act(W . x[r .. r + window - 1, :] + b),   r < rows,
 *   x [rows + window - 1, c_in] with PACKED rows (ld_x == c_in unless window == 1) -- ALL rows + window - 1 rows are
 *   read --, w [n_out, window c_in] with column j c_in + c = the conv weight [:, c, j], y [rows, n_out] (ld_y).  It is
 *   ptgnn_amd_linear_f32 with k = window c_in and overlapping rows: same kernels, same launch counters, same bits.
 * ptgnn_amd_window_weight_grad_f32: grad_w [n_out, window c_in] = sum_r grad_y[r]^T . x[r .. r + window - 1] and grad_b
 *   [n_out] (nullable) = column sums of grad_y, on the kernels of ptgnn_amd_linear_weight_grad_f32 (its constraints:
 *   c_in % 4 == 0, n_out % 4 == 0, 16-byte aligned rows); workspace: ptgnn_amd_edge_wgrad_workspace_bytes(rows, 1, n_out,
 *   window c_in) bytes.
 *
 * ptgnn_amd_window_max_f32 (torch.max(l3_out, dim=-1) at :141): out[b, :] = max over the first `valid` of sample b's
 *   rows_per_sample rows of x (ld_x); arg (nullable, int32 [num_samples, dim] contiguous) = the LOWEST position that
 *   attains it (torch.max's rule; a NaN wins from its first position).  1 <= valid <= rows_per_sample.
 * ptgnn_amd_window_max_backward_f32: writes EVERY row of grad_x [num_samples rows_per_sample, dim] (ld_gx): grad[b, d]
 *   (ld_grad) at row arg[b, d] of sample b, exact zeros elsewhere.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_char_embed_supported(int32_t num_chars, int32_t window, int32_t dim);
int ptgnn_amd_char_embed_f32(const int64_t *chars, int64_t num_samples, int32_t length, int32_t num_chars,
                             int32_t window, const float *table, const float *bias /* nullable */, int32_t dim, int act,
                             float *out, int64_t ld_out, void *stream);
int32_t ptgnn_amd_char_embed_backward_chunk(void);
size_t ptgnn_amd_char_embed_backward_workspace_bytes(int64_t num_samples, int32_t num_chars, int32_t window,
                                                     int32_t dim);
int ptgnn_amd_char_embed_backward_f32(const float *grad, int64_t ld_grad, const float *a1, int64_t ld_a1,
                                      const int64_t *chars, int64_t num_samples, int32_t length, int32_t num_chars,
                                      int32_t window, int32_t dim, int act, float *grad_table,
                                      float *grad_bias /* nullable */, void *workspace, size_t workspace_bytes,
                                      void *stream);
int ptgnn_amd_window_linear_f32(const float *x, int64_t rows, int32_t c_in, int32_t window, int64_t ld_x,
                                const float *w, int32_t n_out, const float *bias /* nullable */, int act, float *y,
                                int64_t ld_y, void *stream);
int ptgnn_amd_window_weight_grad_f32(const float *x, int64_t rows, int32_t c_in, int32_t window, const float *grad_y,
                                     int64_t ld_grad_y, int32_t n_out, float *grad_w, float *grad_b /* nullable */,
                                     void *workspace, size_t workspace_bytes, void *stream);
int ptgnn_amd_window_max_f32(const float *x, int64_t ld_x, int64_t num_samples, int32_t rows_per_sample, int32_t valid,
                             int32_t dim, float *out, int64_t ld_out, int32_t *arg /* nullable */, void *stream);
int ptgnn_amd_window_max_backward_f32(const float *grad, int64_t ld_grad, const int32_t *arg, int64_t num_samples,
                                      int32_t rows_per_sample, int32_t dim, float *grad_x, int64_t ld_gx, void *stream);

/* ------------------------------------------------------------------------------------------
 * Task heads (csrc/task_heads.hip): what the three benchmarked models run after their GNN.  Exact fp32, no float
 * atomics, every sum over rows or slots folded in a fixed order; no entry point synchronises.
 *
 * TOTALS BLOCK, written by every forward call that has targets: PTGNN_AMD_HEAD_TOTALS_BYTES bytes, 8-byte aligned,
 * eight 8-byte slots
 *   slot 0  float64  the loss sum (softmax: sum of lse - logit[target] over live rows; sigmoid: sum over all
 *                    elements; candidates: sum over slots of score[correct] - lse)
 *   slot 1  int64    the denominator of the loss: live rows (softmax), rows (sigmoid), slots (candidates)
 *   slot 2  int64    softmax: rows whose arg-max is their target | sigmoid: true positives  | candidates: slots whose
 *                    arg-max candidate is the correct one
 *   slot 3  int64    softmax: targets outside [0, C) other than -100 | sigmoid: false positives | candidates: correct
 *                    indices that are not a candidate of their slot
 *   slot 4  int64    softmax: 0 | sigmoid: false negatives | candidates: node ids outside [0, num_nodes)
 *   slot 5  int64    rows / candidates of the call;  slots 6, 7: 0
 * The backward entry points read slot 1 from the device; the host never needs it.
 *
 * METRICS BLOCK, optional (NULL: none), PTGNN_AMD_HEAD_METRICS_BYTES bytes, 8-byte aligned, caller-owned and
 * PERSISTENT: the merge step of a forward call ADDS into it, so a module accumulates its metrics over minibatches
 * without a launch of its own and reads them when somebody asks.  The caller zeroes it to reset.
 *   softmax, candidates:  int64 correct | int64 samples (live rows / slots) | int64 skipped targets | unused
 *   sigmoid:              float64 sum precision * rows | float64 sum recall * rows | float64 sum F * rows | int64 rows
 * (precision, recall and F from tp, fp, fn converted to fp32, in the fp32 expression of ppi.py:50-52, 1e-10 terms
 * included).  Like the plan build's control block and the node-id guard's accumulator, a metrics block belongs to ONE
 * stream at a time: calls that add into it from two streams at once race.
 * ---------------------------------------------------------------------------------------- */
#define PTGNN_AMD_HEAD_TOTALS_BYTES 64
#define PTGNN_AMD_HEAD_METRICS_BYTES 32
enum { PTGNN_AMD_LOSS_SOFTMAX = 0, PTGNN_AMD_LOSS_SIGMOID = 1 };

/* Row loss over logits [rows, classes] (ld), any classes >= 1, any rows >= 0 (rows == 0 launches nothing); every
 * logit is read once.
 *
 * mode PTGNN_AMD_LOSS_SOFTMAX replaces nn.CrossEntropyLoss, torch.argmax and torch.softmax + torch.max of
 *   graph2class.py:91-102.  targets: int64 [rows], or NULL (predict: per-row outputs only, no loss, no totals).
 *   Per row: lse [rows] (required; the backward reads it), argmax int64 [rows] (lowest index on ties), max_prob
 *   [rows] = exp(max - lse), row_loss [rows] = lse - logit[target] (all three nullable).  A target outside [0, C)
 *   makes the row an IGNORED row -- no loss, no gradient, not in the denominator, never used as an index; -100 is
 *   nn.CrossEntropyLoss's ignore_index, any other such value is counted in slot 3.  Logits of any spread: a running
 *   maximum.  loss[0] = slot 0 / slot 1 (nan when every row is ignored, as the reference).
 * mode PTGNN_AMD_LOSS_SIGMOID replaces torch.sigmoid(l) >= 0.5, the three masked sums, precision / recall / F and
 *   binary_cross_entropy_with_logits(reduction="none").sum(-1).mean() of ppi.py:43-62.  targets: uint8 [rows,
 *   classes] (ld_t; torch.bool storage), required.  Per element max(l, 0) - l t + log1p(exp(-|l|)), prediction
 *   l >= 0; row_loss [rows] nullable; lse, argmax, max_prob unused.  loss[0] = slot 0 / rows.
 * workspace: ptgnn_amd_logit_loss_workspace_bytes(rows), 8-byte aligned. */
size_t ptgnn_amd_logit_loss_workspace_bytes(int64_t rows);
int ptgnn_amd_logit_loss_f32(const float *logits, int64_t ld, int64_t rows, int32_t classes, int mode,
                             const void *targets /* nullable in mode 0 */, int64_t ld_t, float *lse,
                             int64_t *argmax /* nullable */, float *max_prob /* nullable */,
                             float *row_loss /* nullable */, float *loss, void *totals, void *metrics /* nullable */,
                             void *workspace, size_t workspace_bytes, void *stream);
/* grad_logits [rows, classes] (ld_g), every element written: grad_loss[0] / slot 1 * (exp(l - lse) - onehot), zeros
 * for ignored rows (softmax); grad_loss[0] / rows * (sigmoid(l) - t) (sigmoid).  grad_loss [1] and totals are DEVICE
 * memory: the upstream scalar and the denominator never visit the host. */
int ptgnn_amd_logit_loss_backward_f32(const float *logits, int64_t ld, int64_t rows, int32_t classes, int mode,
                                      const void *targets, int64_t ld_t, const float *lse /* mode 0 */,
                                      const void *totals, const float *grad_loss, float *grad_logits, int64_t ld_g,
                                      void *stream);

/* Candidate scoring of varmisuse.py:63-91 over the segment plan (rowptr int32 [num_slots + 1], perm int32
 * [num_candidates]: the candidates of slot g are perm[rowptr[g] .. rowptr[g + 1])) of the candidate -> slot map
 * cand_slot int64 [num_candidates]:
 *     scores[c] = x[cand_idx[c]] . w[:dim] + x[slot_idx[cand_slot[c]]] . w[dim:]        [num_candidates]
 *     lse[g]    = log sum_{c in g} exp(scores[c])        (-inf for a slot without candidates: eps = 0)
 *     argmax[g] = the POSITION c of the slot's best candidate, lowest on ties, num_candidates for an empty slot
 *                 (what torch_scatter.scatter_max reports)
 *     loss[0]   = -(1 / num_slots) sum_g (scores[correct[g]] - lse[g])
 * replacing the two row gathers, the [num_candidates, 2 dim] torch.cat, nn.Linear(2 dim, 1), scatter_log_softmax and
 * scatter_max: neither the concatenation nor a gathered copy exists.  correct int64 [num_slots] is nullable (scores,
 * lse, argmax only).  correct[g] must be a candidate OF SLOT g (the reference's one-slot-per-graph assumption,
 * varmisuse.py:61): any other value -- outside [0, num_candidates) or a candidate of another slot -- contributes
 * nothing, is counted in slot 3 and never indexes memory.  Node ids outside [0, num_nodes) are clamped and counted
 * (slot 4), like every row gather of the library.
 * Supported: dim a multiple of 4, 4 <= dim <= 1024 (ptgnn_amd_candidate_scores_supported); others answer
 * PTGNN_AMD_EUNSUPPORTED before any device work.  num_slots == 0 launches nothing.
 * workspace: ptgnn_amd_candidate_scores_workspace_bytes(num_slots). */
int ptgnn_amd_candidate_scores_supported(int32_t dim);
size_t ptgnn_amd_candidate_scores_workspace_bytes(int64_t num_slots);
int ptgnn_amd_candidate_scores_f32(const float *x, int64_t ld_x, int64_t num_nodes, const int64_t *cand_idx,
                                   const int64_t *slot_idx, const int64_t *cand_slot, const int32_t *rowptr,
                                   const int32_t *perm, int64_t num_candidates, int64_t num_slots, int32_t dim,
                                   const float *w, const int64_t *correct /* nullable */, float *scores, float *lse,
                                   int64_t *argmax, float *loss, void *totals, void *metrics /* nullable */,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* With t[c] = grad_loss[0] / num_slots * (exp(scores[c] - lse[g]) - [c == correct[g]]) + grad_scores[c]  (g the slot of
 * c; grad_loss [1] on the DEVICE, nullable = 0; grad_scores [num_candidates] nullable = 0; a skipped correct[g] gives
 * its slot no loss gradient):
 *     row_grad[c, :]                  = t[c] w[:dim]                      row_grad is [num_candidates + num_slots, dim],
 *     row_grad[num_candidates + g, :] = (sum_{c in g} t[c]) w[dim:]       the rows of cat(cand_idx, slot_idx)
 *     grad_w[:dim] = sum_c t[c] x[cand_idx[c]],  grad_w[dim:] = sum_g (sum_{c in g} t[c]) x[slot_idx[g]]
 * grad_w from per-slot partials added in slot order.  The host turns row_grad into d x with ONE segment sum over the
 * plan of cat(cand_idx, slot_idx).  Rows of candidates the plan does not hold are not written.
 * workspace: ptgnn_amd_candidate_scores_backward_workspace_bytes(num_slots, dim). */
size_t ptgnn_amd_candidate_scores_backward_workspace_bytes(int64_t num_slots, int32_t dim);
int ptgnn_amd_candidate_scores_backward_f32(const float *x, int64_t ld_x, int64_t num_nodes, const int64_t *cand_idx,
                                            const int64_t *slot_idx, const int64_t *cand_slot, const int32_t *rowptr,
                                            const int32_t *perm, int64_t num_candidates, int64_t num_slots, int32_t dim,
                                            const float *w, const int64_t *correct /* nullable */, const float *scores,
                                            const float *lse, const float *grad_loss /* nullable */,
                                            const float *grad_scores /* nullable */, float *row_grad, float *grad_w,
                                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The loss of the copying decoder (csrc/vocab_loss.hip), replacing ptgnn/neuralmodels/sequence/
 * grucopydecoder.py:118-135, 171-212: the `+ vocab_bias`, torch.logsumexp over cat(target_scores, total_copy_scores),
 * `target_logprobs = target_scores - normalizing_const` [B, L, V], the torch.gather of the correct tokens and, for the
 * third entry, the UNK mask, the stacked logsumexp, the length mask and the two means.  The [B L, V] log-probabilities
 * never exist.  rows = B L decoding locations; s[r, v] = scores[r, v] + bias[v].  Exact fp32, no float atomics, fixed
 * fold orders (two calls give the same bits); rows == 0 launches nothing.
 *
 * ptgnn_amd_vocab_loss_f32: scores [rows, vocab] (ld >= vocab; rows of any alignment) is the raw output of the second
 *   vocabulary Linear, bias [vocab] nullable, extra [rows] nullable (the per-location copy normaliser, -inf for a
 *   sample without memories), targets int64 [rows] nullable.
 *     norm[r]   = logaddexp(log sum_v exp s[r, v], extra[r])     (extra[r] = -inf: the vocabulary term bit for bit)
 *     picked[r] = s[r, targets[r]] - norm[r]                      (targets given; nan for a target outside [0, vocab),
 *                                                                  which is never used as an index)
 *     stats[r]  = (M, log_sum) with norm[r] = M + log_sum: the maximum over the row and extra[r], and the log of the sum
 *                 relative to it ([rows, 2], 8-byte aligned).  The sum norm[r] is rounded at the magnitude of the logits,
 *                 the pair is not: picked and the backward entry work from the pair.
 *   Every score is read once, under a running maximum.  The columns of a row are split over workgroups; the
 *   per-(row, column chunk) partials are merged in chunk order.
 * ptgnn_amd_vocab_loss_backward_f32: stats [rows, 2] of the forward; g_norm [rows], g_picked [rows] DEVICE memory,
 *   nullable = 0.
 *     grad_scores[r, v] = (g_norm[r] - g_picked[r]) exp(s[r, v] - norm[r]) + g_picked[r] [v == targets[r]]     (ld_g)
 *     grad_extra[r]     = (g_norm[r] - g_picked[r]) exp(extra[r] - norm[r])       nullable; 0 for extra[r] = -inf
 *     grad_bias[v]      = sum_r grad_scores[r, v]                                 nullable
 *   One pass: scores read once, gradients written once, grad_bias from per-row-block partials of that pass added in
 *   row-block order (workspace; needed only with grad_bias, 16-byte aligned).
 * ptgnn_amd_copy_loss_finish_f32 (grucopydecoder.py:171-212, after the two per-location terms exist): gen [B L] the
 *   picked generation log-probabilities, copied [B L] the per-location log-sum-exp of the correct copy log-probabilities
 *   (-inf: nothing to copy), rowptr int32 [B L + 1] nullable: the row pointer of the plan of
 *   copyable_elements_sample_idxs over the locations (a location has a copy when its row is not empty), targets int64
 *   [B L], lengths int64 [B].
 *     gen'    = has_copy && targets == unk_id ? -inf : gen
 *     any     = logsumexp(stack(gen', copied))
 *     loss[0] = -mean_b( sum_{l} any[b, l] * [l < lengths[b]] / sum_l [l < lengths[b]] )
 *   in the reference's arithmetic (the mask is a product; steps in step order, samples in sample order), and d_gen,
 *   d_copied [B L] = d loss / d gen, d loss / d copied (0 where masked or -inf).  One launch of one workgroup.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_vocab_loss_workspace_bytes(int64_t rows, int32_t vocab);
int ptgnn_amd_vocab_loss_f32(const float *scores, int64_t ld, int64_t rows, int32_t vocab,
                             const float *bias /* nullable */, const float *extra /* nullable */,
                             const int64_t *targets /* nullable */, float *norm, float *picked /* with targets */,
                             float *stats, void *workspace, size_t workspace_bytes, void *stream);
size_t ptgnn_amd_vocab_loss_backward_workspace_bytes(int64_t rows, int32_t vocab);
int ptgnn_amd_vocab_loss_backward_f32(const float *scores, int64_t ld, int64_t rows, int32_t vocab,
                                      const float *bias /* nullable */, const float *extra /* nullable */,
                                      const int64_t *targets /* nullable */, const float *stats,
                                      const float *g_norm /* nullable */, const float *g_picked /* nullable */,
                                      float *grad_scores, int64_t ld_g, float *grad_extra /* nullable */,
                                      float *grad_bias /* nullable */, void *workspace, size_t workspace_bytes,
                                      void *stream);
size_t ptgnn_amd_copy_loss_finish_workspace_bytes(int64_t num_samples);
int ptgnn_amd_copy_loss_finish_f32(const float *gen, const float *copied, const int32_t *rowptr /* nullable */,
                                   const int64_t *targets, int64_t unk_id, const int64_t *lengths, int64_t num_samples,
                                   int32_t steps, float *loss, float *d_gen, float *d_copied, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * One step of the copying decoder's greedy decoding (csrc/decode_step.hip), replacing the per-step host work of
 * ptgnn/neuralmodels/sequence/grucopydecoder.py:375-457: `target_logprobs`, torch.topk, the three .cpu() copies, the
 * Python dict merge of copy and vocabulary probabilities, the arg-max and the next token tensor.  One launch, one
 * workgroup per sample, no host read-back; the [B, V] log-probabilities never exist.
 *   scores [B, vocab] (ld >= vocab) the RAW output of the second vocabulary Linear, bias [vocab] nullable,
 *   copy_scores [num_memories] and total_copy [B] (their per-sample log-sum-exp, -inf for a sample without memories) as
 *   ptgnn_amd_segment_scores_f32 leaves them for one vector per sample.
 *   The value grouping of the call: rowptr int32 [B + 1], slot_memory int32 [num_memories] (the memory of a slot) and
 *   slot_ids int64 [num_memories] (its value id), the slots of sample b being rowptr[b] .. rowptr[b + 1] - 1 with
 *   ascending ids.  An id < vocab is a vocabulary id; any other id is the caller's key of an out-of-vocabulary value.
 * Per sample b with done[b] == 0, s[v] = scores[b, v] + bias[v] and norm = logaddexp(log sum_v exp s[v], total_copy[b]):
 *   every run of equal ids g is an entry  log sum_{slots of the run} exp(copy_scores[.] - norm), merged by logaddexp with
 *   s[g] - norm when g < vocab and s[g] is one of the top_k largest of the row; the other entry is the row's largest,
 *   s[v*] - norm.  The prediction is the largest entry.  Exact ties: among equal scores of the row the lower index is
 *   the larger (top-1 and the top_k-th place alike), the row's entry goes before a run of equal value, and of two runs
 *   the lower id.
 *     logprobs[b] += the entry;  prediction == end_id: done[b] = 1;  else tokens[b, step] = prediction, lengths[b] += 1
 *     next_tokens[b] = prediction < vocab ? prediction : unk_id
 * A sample with done[b] != 0 gets next_tokens[b] = end_id and nothing else.  tokens is [B, max_steps].
 * slot_memory entries outside [0, num_memories) and negative ids are clamped to 0 and counted in bad[0] (int32, DEVICE
 * memory, nullable), like every row gather of the library.  Exact fp32, no float atomics: two calls give the same
 * bits.  vocab < 1, top_k < 1, a step outside [0, max_steps) or unk_id / end_id outside the vocabulary answer
 * PTGNN_AMD_EINVAL before any device work; num_samples == 0 launches nothing.
 * workspace: ptgnn_amd_decode_step_workspace_bytes(num_samples, vocab, top_k) -- 0 today (a sample's partial results stay
 * in the LDS of its workgroup), 0 for sizes the entry refuses.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_decode_step_workspace_bytes(int64_t num_samples, int32_t vocab, int32_t top_k);
int ptgnn_amd_decode_step_f32(const float *scores, int64_t ld, const float *bias /* nullable */,
                              const float *copy_scores, const float *total_copy, const int32_t *slot_memory,
                              const int32_t *rowptr, const int64_t *slot_ids, int64_t num_samples,
                              int64_t num_memories, int32_t vocab, int32_t top_k, int64_t unk_id, int64_t end_id,
                              int32_t step, int32_t max_steps, int32_t *done, int64_t *lengths, float *logprobs,
                              int64_t *tokens, int64_t *next_tokens, int32_t *bad /* nullable */, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * One step of the copying decoder's beam search (csrc/beam_step.hip): the step above widened from the best entry of a
 * sample to the W = beam_width best continuations of its W hypotheses ("slots").  The reference has no beam search; the
 * semantics extend its greedy dictionary (grucopydecoder.py:406-442) and equal the step above for W = 1.  No host
 * read-back; the [B W, V] log-probabilities never exist.
 *   scores [B W, vocab] (ld >= vocab; row b W + j is slot j of sample b), bias [vocab] nullable, copy_scores
 *   [num_memories, W] and total_copy [B, W] as ptgnn_amd_segment_scores_f32 leaves them for W vectors per sample, the
 *   value grouping (rowptr, slot_memory, slot_ids) of the step above.
 *   The state IN: beam_scores_in float [B, W], done_in int32 [B, W], lengths_in int64 [B, W], tokens_in int64
 *   [B, W, max_steps]; the state OUT in buffers of the same shapes that do not overlap them (slots are reordered: the
 *   caller swaps the two sets between steps); next_tokens int64 [B W]; parent_rows int64 [B W] = b W + parent of the slot,
 *   the index of the row gather that reorders the hidden states.
 * Per sample, slot j with done_in == 0 has the ENTRIES of the step above, from its own row, its own column of the copy
 * scores and norm_j: the top_k largest s_j[v] - norm_j, merged with every run of equal ids (onto the vocabulary entry
 * where g < vocab and s_j[g] is one of the top_k, else onto -inf).  Entry e is the candidate (parent j, id e, score
 * beam_scores_in[j] + entry); a slot with done_in != 0 is one candidate, itself, score unchanged.  The W candidates of the
 * sample that come first in this order become the slots 0 .. W - 1 of the state out, in that order:
 *   1. higher score;  2. lower parent;  3. inside a parent the entries whose id is one of its W best vocabulary columns
 *   (of equal scores of a row the lower index is the larger, as above) before its other entries;  4. lower id.
 * Candidates that are all -inf are ordered by 2.-4. for a parent whose score is finite; a live parent whose score is
 * -inf (slots 1 .. W - 1 before the first step) offers the ids 0 .. W - 1 at -inf without a look at its row -- with
 * beam_width <= min(top_k, vocab) and finite scores at least W candidates are finite and these are never taken.
 *   id == end_id: done_out = 1, the score includes END's entry, nothing is appended;  a finished parent: copied;
 *   otherwise tokens_out[.., step] = id after the parent's history, lengths_out = lengths_in[parent] + 1.
 *   next_tokens = end_id for a finished slot, else id < vocab ? id : unk_id.
 * slot_memory entries outside [0, num_memories) and negative ids are clamped to 0 and counted in bad[0] (int32, DEVICE
 * memory, nullable), once per slot and call.  Exact fp32, no float atomics, fixed fold orders: two calls give the same
 * bits.  Before any device work: vocab < 1, top_k < 1, beam_width outside [1, 8] or above min(top_k, vocab), a step
 * outside [0, max_steps), unk_id / end_id outside the vocabulary, a null required pointer or a workspace below
 * ptgnn_amd_beam_step_workspace_bytes(...) answer PTGNN_AMD_EINVAL, sizes beyond int32 indexing PTGNN_AMD_EUNSUPPORTED;
 * num_samples == 0 launches nothing.  The workspace holds one float per (memory, slot) and the W W candidates of every
 * sample between the two kernels of the entry; its size is 0 for sizes the entry refuses.
 * ---------------------------------------------------------------------------------------- */
size_t ptgnn_amd_beam_step_workspace_bytes(int64_t num_samples, int64_t num_memories, int32_t vocab, int32_t top_k,
                                           int32_t beam_width);
int ptgnn_amd_beam_step_f32(const float *scores, int64_t ld, const float *bias /* nullable */, const float *copy_scores,
                            const float *total_copy, const int32_t *slot_memory, const int32_t *rowptr,
                            const int64_t *slot_ids, int64_t num_samples, int64_t num_memories, int32_t vocab,
                            int32_t top_k, int32_t beam_width, int64_t unk_id, int64_t end_id, int32_t step,
                            int32_t max_steps, const float *beam_scores_in, const int32_t *done_in,
                            const int64_t *lengths_in, const int64_t *tokens_in, float *beam_scores_out,
                            int32_t *done_out, int64_t *lengths_out, int64_t *tokens_out, int64_t *next_tokens,
                            int64_t *parent_rows, int32_t *bad /* nullable */, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ------------------------------------------------------------------------------------------
 * The finishing route of the beam search (csrc/beam_step.hip): length normalisation, back-pointers in place of copied
 * histories, and a count of the live slots that lets the host leave its loop early.  Two entries beside the step above,
 * which keeps its code and its bits.  (The names say "search" and "greedy": the symbol sets of the two steps above are
 * closed.)
 *
 * ptgnn_amd_search_step_links_f32: the step above without tokens_in / tokens_out, with
 *   key_scale float [max_steps + 1], every entry > 0: a candidate whose parent has lengths_in == l is PLACED by
 *     key = score * key_scale[l + 1] in place of rule 1. (higher key; 2.-4. as above).  l + 1 counts the scored decisions
 *     of the candidate -- the appended tokens, plus END's once it has finished -- and is the same for every candidate of a
 *     parent, a finished parent standing for itself included, so the order inside a parent is that of the raw sums.  The
 *     host makes the table (GNMT: ((5 + n) / 6) ** -alpha, in double, rounded once); nothing is raised to a power or
 *     divided on the device.  -inf stays -inf and a nan never compares first.  beam_scores_out holds the RAW sums, in key
 *     order: with a table that is not all ones they need not descend.  An all-ones table gives the bits of the step above.
 *   links int32 [max_steps, B, W, 2]: slot p of sample b writes links[step, b, p] = (the id it appends, or -1 where it
 *     is or becomes finished; its parent slot 0 .. W - 1).  Ids fit: element keys are below 2 ** 22, vocabulary ids below
 *     the int32 limit the entry enforces.
 *   live int32 [max_steps], nullable, zeroed by the caller once per call: the number of slots of the sample with
 *     done_out == 0 is added to live[step], one integer atomic per sample.  Once live[s] == 0 every later step is the
 *     identity (a finished slot is its own single candidate, its key does not change, the slots are in selection order).
 *   The workspace is that of the step above: ptgnn_amd_beam_step_workspace_bytes(...).
 * ptgnn_amd_search_backtrack: one launch per call, after the loop.  For every final slot (b, w) it walks
 *   s = steps_run - 1 .. 0 through links: tokens[b, w, s] = id, slot = parent; and writes -1 at every column
 *   >= steps_run, so tokens int64 [B, W, max_steps] needs no fill.  A token appended at step s sits at column s, because a
 *   live hypothesis has appended at every earlier step: no length arithmetic.  Cost: one thread per final slot, a chain
 *   of steps_run DEPENDENT 8-byte loads each, once per call, against 16 max_steps B W bytes of copied histories per STEP.
 * Both: exact fp32, integer atomics only, fixed fold orders -- two calls give the same bits.  Before any device work a
 * null key_scale / links / tokens, steps_run outside [0, max_steps] and the size conditions of the step above answer
 * PTGNN_AMD_EINVAL, sizes beyond int32 indexing (2 B W max_steps pairs included) PTGNN_AMD_EUNSUPPORTED; num_samples == 0
 * launches nothing.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_search_step_links_f32(const float *scores, int64_t ld, const float *bias /* nullable */,
                                    const float *copy_scores, const float *total_copy, const int32_t *slot_memory,
                                    const int32_t *rowptr, const int64_t *slot_ids, int64_t num_samples,
                                    int64_t num_memories, int32_t vocab, int32_t top_k, int32_t beam_width, int64_t unk_id,
                                    int64_t end_id, int32_t step, int32_t max_steps, const float *key_scale,
                                    const float *beam_scores_in, const int32_t *done_in, const int64_t *lengths_in,
                                    float *beam_scores_out, int32_t *done_out, int64_t *lengths_out, int64_t *next_tokens,
                                    int64_t *parent_rows, int32_t *links, int32_t *live /* nullable */,
                                    int32_t *bad /* nullable */, void *workspace, size_t workspace_bytes, void *stream);
int ptgnn_amd_search_backtrack(const int32_t *links, int64_t num_samples, int32_t beam_width, int32_t steps_run,
                               int32_t max_steps, int64_t *tokens, void *stream);

/* ------------------------------------------------------------------------------------------
 * The greedy-decoding step (csrc/decode_step.hip, ptgnn_amd_decode_step_f32: the same kernel, arguments, checks, bits and
 * counter family) with live int32 [max_steps], required, zeroed by the caller once per call: a sample that is not done
 * AFTER the step adds 1 to live[step] (an integer atomic).  live[s] == 0: every later step changes nothing but
 * next_tokens, and the host may leave its loop.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_greedy_step_live_f32(const float *scores, int64_t ld, const float *bias /* nullable */,
                                   const float *copy_scores, const float *total_copy, const int32_t *slot_memory,
                                   const int32_t *rowptr, const int64_t *slot_ids, int64_t num_samples,
                                   int64_t num_memories, int32_t vocab, int32_t top_k, int64_t unk_id, int64_t end_id,
                                   int32_t step, int32_t max_steps, int32_t *done, int64_t *lengths, float *logprobs,
                                   int64_t *tokens, int64_t *next_tokens, int32_t *live, int32_t *bad /* nullable */,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the GGNN layer's dense blocks (csrc/half_gemm.hip).
 *
 * Replaces: what an `enable_amp` user of the reference trainer gets (ptgnn/baseneuralmodel/trainer.py:205,221: the
 *   forward runs under torch.cuda.amp.autocast, so the message Linears and the GRU cell of gatedmessagepassing.py:57-69
 *   take their operands in the autocast dtype; the reference up-casts only at the scatter,
 *   abstractmessagepassing.py:43-50).  OFF by default: nothing in the library calls these entries unless the host's
 *   ptgnn_amd.precision setting asks for it; this is not a GEMM mode (ptgnn_amd_set_gemm_mode is unchanged).
 *
 * States stay fp32 in memory.  The kernels round x / a / h to `dtype` (PTGNN_AMD_HALF_BF16 / _F16) in registers, to
 * nearest even, exactly as tensor.to(dtype) does; the weights arrive ALREADY rounded as 16-bit arrays in the nn.Linear /
 * nn.GRUCell layouts (the host makes them with tensor.to(dtype)).  Products run on v_mfma_f32_32x32x16_{bf16,f16};
 * accumulation, bias, activation, gate math and the stores are fp32:
 *   ptgnn_amd_half_linear  : y = act(rnd(x) rnd(W)^T + b); x [rows, k] (ld_x), w 16-bit [n_out, k], bias fp32 [n_out]
 *     (nullable), y [rows, n_out] (ld_y), act = PTGNN_AMD_ACT_* as ptgnn_amd_linear_f32.
 *   ptgnn_amd_half_gru_cell: gi = rnd(a) rnd(W_ih)^T + b_ih, gh = rnd(h) rnd(W_hh)^T + b_hh, r = sigmoid(gi_r + gh_r),
 *     z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h with the UNROUNDED fp32 h in the blend.
 *     Shapes as ptgnn_amd_gru_cell_f32, w_ih / w_hh 16-bit; `out` has its own ld_out (a column slice of a wider buffer is
 *     fine); out != h.  Gate math: the streaming fp32 cell's expressions, so both cells meet the same bar against a
 *     float64 reference on the rounded operands.
 *   ptgnn_amd_half_supported(kind, k_or_m, n_out_or_hd, dtype): 1 when the kernels take the shape, else 0; needs no
 *     device.  kind PTGNN_AMD_HALF_KIND_LINEAR: k % 32 == 0, k <= 1024, n_out % 32 == 0.  _GRU: m % 32 == 0,
 *     hd % 32 == 0, both <= 1024.
 * Any number of rows, 0 included (no launch).  x, a, h and the weights must be 16-byte aligned with ld % 4 == 0; y, out
 * and the biases aligned to a float.  A bad dtype / act / size or a null pointer answers PTGNN_AMD_EINVAL, a shape or an
 * alignment outside the above PTGNN_AMD_EUNSUPPORTED, both with a message and before anything touches the device.
 * Row independence: the bits of output row r depend on row r of the inputs and on the weights only -- not on `rows`,
 * the launch geometry or the row's position; a launch over [0, n) equals launches over any partition of it.
 * Magnitudes below the 16-bit type's smallest normal (bf16: 2^-126, fp16: 2^-14) are outside the contract (whether
 * they flush follows the hardware's denormal mode, not torch's); fp16 overflow becomes inf, as tensor.half() gives.
 * No float atomics: two calls give the same bits.
 * ---------------------------------------------------------------------------------------- */
enum { PTGNN_AMD_HALF_BF16 = 1, PTGNN_AMD_HALF_F16 = 2 };
enum { PTGNN_AMD_HALF_KIND_LINEAR = 0, PTGNN_AMD_HALF_KIND_GRU = 1 };
int ptgnn_amd_half_supported(int kind, int32_t k_or_m, int32_t n_out_or_hd, int dtype);
int ptgnn_amd_half_linear(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w, int32_t n_out,
                          const float *bias /* nullable */, int act, int dtype, float *y, int64_t ld_y, void *stream);
int ptgnn_amd_half_gru_cell(const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                            const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m, int32_t hd,
                            int dtype, float *out, int64_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the GGNN TRAINING step (csrc/wgrad16.hip, csrc/half_gemm.hip).
 *
 * Replaces: the backward of the message Linears and of the GRU cell of gatedmessagepassing.py:57-69 under the
 *   reference trainer's `enable_amp` (trainer.py:205,221: autocast runs them in the 16-bit type forward AND backward).
 *   OFF by default: the host's ptgnn_amd.precision setting asks for it with `training=True`.
 *
 * Semantics.  States, saved tensors, gradients, accumulation, bias, gate math and gate-math backward stay fp32; only
 * GEMM operands are rounded, to nearest even as tensor.to(dtype) does -- in registers, or by torch for the weights:
 *   Linear y = x W^T + b: forward rnd(x) rnd(W)^T + b (ptgnn_amd_half_linear); d_x = rnd(g) rnd(W)
 *     (ptgnn_amd_half_linear on the rounded TRANSPOSED weights); d_W = rnd(g)^T rnd(x) (ptgnn_amd_linear_weight_grad16);
 *     d_b = column sums of the UNROUNDED fp32 g.
 *   GRU cell: forward ptgnn_amd_gru_cell_train16 = ptgnn_amd_half_gru_cell (bit-equal `out`) that also writes
 *     gates [n, 4 hd] = r | z | n | gh_n, the fp32 values its gate math used; d_gi, d_gh, d_h from the fp32
 *     ptgnn_amd_gru_cell_backward_gates_f32; d_a = rnd(d_gi) rnd(W_ih); d_h + rnd(d_gh) rnd(W_hh) in one launch
 *     (ptgnn_amd_linear_add16); d_W_ih = rnd(d_gi)^T rnd(a), d_W_hh = rnd(d_gh)^T rnd(h); the bias gradients are
 *     column sums of the fp32 d_gi, d_gh.
 *   fp16 overflow of a rounded gradient becomes inf, as tensor.half() gives (GradScaler expects it).
 *
 *   ptgnn_amd_linear_weight_grad16: grad_w [n_out, k] = rnd(grad_y)^T rnd(x), x [rows, k] (ld_x), grad_y [rows, n_out]
 *     (ld_grad_y), both fp32 and rounded in the kernel; grad_b [n_out] (nullable) = column sums of the fp32 grad_y from
 *     the same pass.  Every workgroup writes one fp32 partial tile to `workspace`
 *     (ptgnn_amd_wgrad16_workspace_bytes(rows, n_out, k) bytes, 16-byte aligned); a second launch adds the partials in
 *     a fixed order.  Any row count; rows == 0 gives zeros and launches no kernel.
 *   ptgnn_amd_wgrad16_chunk_rows(rows, n_out, k): the rows one workgroup partial covers (ceil(rows / it) partials);
 *     needs no device; 0 for a shape the kernel does not take.
 *   ptgnn_amd_half_supported(PTGNN_AMD_HALF_KIND_WGRAD, k, n_out, dtype): k % 32 == 0, n_out % 32 == 0, both <= 1024.
 *     (The kind's id is 3: id 2 stays an unknown kind, as it has always answered.)
 *   ptgnn_amd_gru_cell_train16: arguments of ptgnn_amd_half_gru_cell plus `gates` (contiguous [n, 4 hd]).  Row
 *     independence as documented for ptgnn_amd_half_gru_cell.
 *   ptgnn_amd_linear_add16: ptgnn_amd_half_linear plus an fp32 `addend` [rows, n_out] (ld_add) added after the
 *     activation in the store epilogue: y = act(rnd(x) rnd(W)^T + b) + addend.
 * x, grad_y, a, h, the weights, grad_w, grad_b and the workspace must be 16-byte aligned with ld % 4 == 0; the other
 * outputs, the addend and the biases aligned to a float.  Error codes as ptgnn_amd_half_linear, messages starting with
 * "linear_weight_grad16:", "gru_cell_train16:", "linear_add16:", before anything touches the device.
 * No float atomics anywhere: two calls give the same bits.
 * (The entries carry a "16" suffix like ptgnn_amd_edge_linear16: the ptgnn_amd_half_* prefix is a closed set of three.)
 * ---------------------------------------------------------------------------------------- */
enum { PTGNN_AMD_HALF_KIND_WGRAD = 3 };
int ptgnn_amd_linear_weight_grad16(const float *x, int64_t ld_x, int32_t k, const float *grad_y, int64_t ld_grad_y,
                                   int64_t rows, int32_t n_out, int dtype, float *grad_w,
                                   float *grad_b /* nullable */, void *workspace, size_t workspace_bytes, void *stream);
size_t ptgnn_amd_wgrad16_workspace_bytes(int64_t rows, int32_t n_out, int32_t k);
int64_t ptgnn_amd_wgrad16_chunk_rows(int64_t rows, int32_t n_out, int32_t k);
int ptgnn_amd_gru_cell_train16(const float *a, int64_t ld_a, const float *h, int64_t ld_h, const void *w_ih,
                               const void *w_hh, const float *b_ih, const float *b_hh, int64_t n, int32_t m, int32_t hd,
                               int dtype, float *out, int64_t ld_out, float *gates, void *stream);
int ptgnn_amd_linear_add16(const float *x, int64_t rows, int32_t k, int64_t ld_x, const void *w, int32_t n_out,
                           const float *bias /* nullable */, int act, int dtype, const float *addend, int64_t ld_add,
                           float *y, int64_t ld_y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the GGNN layer's grouped per-edge GEMM (csrc/edge_gemm16.hip).
 *
 * Replaces: the message Linears of gatedmessagepassing.py:50-61 under autocast, where the minibatch takes the edge form
 *   (ptgnn_amd_edge_linear_f32 / ptgnn_amd_edge_linear_shared_f32 are the fp32 launches and stay as they are).  OFF by
 *   default: the host's ptgnn_amd.precision setting asks for it with `edge_gemm=True`.
 *
 *   msg[r] = act(rnd(x[src[r]]) rnd(W_t)^T) for every message row r of edge type t; no bias.  x fp32 [num_rows, state_dim]
 *   (ld_x), gathered ids clamped into [0, num_rows); w = ONE 16-bit [num_types, msg_dim, state_dim] stack ALREADY rounded
 *   by the host (tensor.to(dtype)); the gathered rows are rounded to `dtype` (PTGNN_AMD_HALF_BF16 / _F16) in registers, to
 *   nearest even; products on v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation, fp32 msg [rows, msg_dim] (ld_msg).
 *   ptgnn_amd_edge_linear16       : one row per edge in type-major order; src_per_type / edges_per_type are HOST arrays
 *     (device id pointers, counts) as ptgnn_amd_edge_linear_f32 takes them without a target-state half.  No edges: no
 *     launch, PTGNN_AMD_OK.
 *   ptgnn_amd_edge_linear16_shared: one row per distinct (type, source) pair; `edge_table` is the device-resident table
 *     ptgnn_amd_unique_sources wrote on the same stream, as ptgnn_amd_edge_linear_shared_f32 takes it: no host
 *     synchronisation, no read-back (a table without rows launches workgroups that leave at once).
 *   ptgnn_amd_edge_linear16_supported(state_dim, msg_dim, num_types, dtype): 1 when the kernels take the shape, else 0;
 *     needs no device.  state_dim % 32 == 0, msg_dim % 32 == 0, both <= 1024, 2 <= num_types <= 64.
 * x and w must be 16-byte aligned with ld_x % 4 == 0, msg aligned to a float.  A bad dtype / act / size or a null
 * pointer answers PTGNN_AMD_EINVAL, a shape, an alignment or a row count beyond the int32 unit / key range
 * PTGNN_AMD_EUNSUPPORTED, all with a message that starts "edge_linear16:" and before anything touches the device.
 * Row independence: a row's K chain is k ascending in steps of 16 into one accumulator; the bits of message row r
 * depend on x[src[r]] and W_t only -- not on the launch form, the row's position, the number of rows or the workgroup
 * count -- so the aggregate of the shared form equals the aggregate of the per-edge form bit for bit.  Small magnitudes
 * and fp16 overflow: as ptgnn_amd_half_linear.  No atomics: two calls give the same bits.
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_edge_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype);
int ptgnn_amd_edge_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                            const int64_t *const *src_per_type, const int64_t *edges_per_type, const void *w,
                            int32_t num_types, int32_t msg_dim, int act, int dtype, float *msg, int64_t ld_msg,
                            void *stream);
int ptgnn_amd_edge_linear16_shared(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                   const void *edge_table, const void *w, int32_t num_types, int32_t msg_dim, int act,
                                   int dtype, float *msg, int64_t ld_msg, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the MLP-MP layer's grouped per-edge GEMM: the form WITH a target-state half
 * (csrc/edge_gemm16.hip; the same two kernels as ptgnn_amd_edge_linear16, with a second id list per unit).
 *
 * Replaces: the single-Linear, bias-free edge transforms of mlpmessagepassing.py:88-98 under autocast
 *   (`use_target_state_as_message_input=True`, no edge features), where the minibatch takes the edge form
 *   (ptgnn_amd_edge_linear_f32 with dst_per_type is the fp32 launch and stays as it is).  OFF by default: the host's
 *   ptgnn_amd.precision setting asks for it with `mlp=True`.  Without a target-state half the layer calls
 *   ptgnn_amd_edge_linear16.
 *
 *   msg[r] = act( rnd(x[src[r]]) rnd(W_t[:, :H])^T + rnd(x[dst[r]]) rnd(W_t[:, H:2H])^T )      (H = state_dim)
 *   for every message row r of edge type t, one row per edge in type-major order; no bias.  x, the ids, the counts, msg,
 *   act and dtype as ptgnn_amd_edge_linear16 takes them, plus dst_per_type (a HOST array of device id pointers like
 *   src_per_type); both id lists are clamped into [0, num_rows).  w = ONE 16-bit [num_types, msg_dim, 2 state_dim] stack
 *   ALREADY rounded by the host.  No edges: no launch, PTGNN_AMD_OK.  There is no shared-row form: with a target half a
 *   message row belongs to one edge.
 *   ptgnn_amd_edge_dst_linear16_supported(state_dim, msg_dim, num_types, dtype): 1 when the kernels take the shape, else
 *     0; needs no device.  state_dim % 32 == 0, msg_dim % 32 == 0, both <= 1024, 2 <= num_types <= 64.
 * Alignment and error codes as ptgnn_amd_edge_linear16; every message starts "edge_linear16: dst:" and answers before
 * anything touches the device.
 * Row independence: a row's K chain is one accumulator per 32-column tile, zeroed, k ascending in steps of 16 over the
 * source half and then over the target half; the bits of message row r depend on x[src[r]], x[dst[r]] and W_t only --
 * not on the kernel, the row's position in its 32-row unit, the number of rows or the workgroup count.  Small magnitudes
 * and fp16 overflow: as ptgnn_amd_half_linear.  No atomics: two calls give the same bits.
 * (The names put "dst" before "linear16": the ptgnn_amd_edge_linear16* prefix is a closed set of three, and the ABI
 * version stays -- the entries are additive, like every 16-bit entry before them.)
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_edge_dst_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype);
int ptgnn_amd_edge_dst_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                const int64_t *const *src_per_type, const int64_t *const *dst_per_type,
                                const int64_t *edges_per_type, const void *w, int32_t num_types, int32_t msg_dim,
                                int act, int dtype, float *msg, int64_t ld_msg, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the GGNN layer's edge-form TRAINING step: the grouped per-edge GEMM with the
 * per-edge dropout mask (csrc/edge_gemm16.hip: the same two kernels as ptgnn_amd_edge_linear16, with a compile-time mask
 * mode) and the per-type weight gradient (csrc/edge_wgrad16.hip).
 *
 * Replaces: `edge_transformation_layer(self.__dropout(message_input))` of gatedmessagepassing.py:57-61 under autocast
 *   in training, and its autograd (ptgnn_amd_edge_linear_masked_f32 / ptgnn_amd_edge_weight_grad_masked_f32 and the
 *   other fp32 launches stay as they are).  OFF by default: the host's ptgnn_amd.precision setting asks for it with
 *   `edge_training=True`.
 *
 * ptgnn_amd_edge_masked_linear16: the arguments of ptgnn_amd_edge_linear16 (no target-state half, no activation) plus
 *   (dropout_mode, dropout_p, mask_bits).  mask_bits: the keep mask as bits exactly as ptgnn_amd_edge_linear_masked_f32
 *   takes it (ptgnn_amd_dropout_bitmask; [message rows][width / 32] dwords, bit b of dword c = column 32 c + b; width =
 *   state_dim in mode 1, msg_dim in mode 2); scale = 1.0f / (1.0f - dropout_p) in fp32, dropout_p == 0 means mode 0.
 *     mode 1 (the forward)       : msg[r] = rnd(keep ? x[src[r]] * scale : 0) rnd(W_t)^T -- mask and fp32 scale BEFORE the
 *       one rounding, as autocast applies nn.Dropout before the 16-bit Linear;
 *     mode 2 (the input gradient): out[r] = (rnd(x[r]) rnd(W_t)^T) * keep * scale -- x the incoming gradient over an
 *       identity index, w the rounded TRANSPOSED [num_types, state_dim_fwd, msg_dim_fwd] stack; mask and scale on the
 *       fp32 accumulator, before the store;
 *     mask_bits == NULL or mode 0: the launch and the bits of ptgnn_amd_edge_linear16 on the same arguments.
 *   ptgnn_amd_edge_masked_linear16_supported(state_dim, msg_dim, num_types, dtype, mode): mode 1 or 2, the width the mask
 *     covers a multiple of 32, and otherwise the limits of ptgnn_amd_edge_linear16_supported.  Needs no device.
 *   Alignment and error codes as ptgnn_amd_edge_linear16 (mask_bits 4-byte aligned); every message starts
 *   "edge_linear16: masked:" and answers before anything touches the device.  Row independence as there: the bits of
 *   output row r depend on x[src[r]], W_t and the row's keep bits only -- with dropout_p == 0 a training forward has
 *   the bits of the inference per-edge launch.
 *
 * ptgnn_amd_edge_weight_grad16: grad_w[t] = rnd(g_t)^T rnd(keep ? x[src_t[e]] * scale : 0) for every type in one launch,
 *   fp32 [num_types, msg_dim, state_dim]; g_t = the type's rows of grad_msg [edges, msg_dim] (ld_grad_msg) in type-major
 *   order; ids clamped into [0, num_rows), num_rows < 2^31.  Both fp32 operands are rounded in the kernel, the mask and
 *   the fp32 scale applied before the rounding; mask_bits (the mode-1 mask) is nullable: without it, or with
 *   dropout_p == 0, nothing is dropped and scale = 1.  A type without edges gets zeros.  Deterministic: a type's chunks
 *   of ptgnn_amd_edge_wgrad16_chunk_edges(num_edges, num_types, msg_dim, state_dim) edges (a chunk never crosses a type)
 *   each write one partial into the workspace (ptgnn_amd_edge_wgrad16_workspace_bytes(...) bytes, 16-byte aligned) and a
 *   second launch adds them in a fixed order; no atomics -- two calls give the same bits.
 *   ptgnn_amd_edge_weight_grad16_supported(state_dim, msg_dim, num_types, dtype): state_dim % 32 == 0, msg_dim % 32 == 0,
 *     both <= 1024, 2 <= num_types <= 64.  Needs no device; the two size queries answer 0 for other shapes.
 *   x, grad_msg, grad_w and the workspace must be 16-byte aligned with ld % 4 == 0.  Error codes as above; every message
 *   starts "edge_weight_grad16:".
 * (The names keep "linear16" last, like ptgnn_amd_edge_dst_linear16: the ptgnn_amd_edge_linear16* prefix is a closed set
 * of three.  The entries are additive and the ABI version stays.)
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_edge_masked_linear16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype,
                                             int dropout_mode);
int ptgnn_amd_edge_masked_linear16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                   const int64_t *const *src_per_type, const int64_t *edges_per_type, const void *w,
                                   int32_t num_types, int32_t msg_dim, int dtype, float *msg, int64_t ld_msg,
                                   int dropout_mode, float dropout_p, const uint32_t *mask_bits /* nullable */,
                                   void *stream);
int ptgnn_amd_edge_weight_grad16_supported(int32_t state_dim, int32_t msg_dim, int32_t num_types, int dtype);
int64_t ptgnn_amd_edge_wgrad16_chunk_edges(int64_t num_edges, int32_t num_types, int32_t msg_dim, int32_t state_dim);
size_t ptgnn_amd_edge_wgrad16_workspace_bytes(int64_t num_edges, int32_t num_types, int32_t msg_dim, int32_t state_dim);
int ptgnn_amd_edge_weight_grad16(const float *x, int64_t ld_x, int64_t num_rows, int32_t state_dim,
                                 const int64_t *const *src_per_type, const int64_t *edges_per_type,
                                 const float *grad_msg, int64_t ld_grad_msg, int32_t num_types, int32_t msg_dim,
                                 int dtype, float dropout_p, const uint32_t *mask_bits /* nullable */, float *grad_w,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Opt-in 16-bit matrix-core inputs for the block attention's inference forward (csrc/block_attention16.hip).
 *
 * Replaces: selfattmessagepassing.py:104-117 under autocast -- both einsums ("khd,vhd->khv" of line 107 and
 *   "khv,vhd->khd" of line 112) in the autocast dtype, the softmax of line 110 in fp32 -- for inference (no dropout:
 *   line 111 is the identity in eval()).  ptgnn_amd_block_attention_f32 is the fp32 launch and stays as it is.  OFF by
 *   default: the host's ptgnn_amd.precision setting asks for it with `attention=True`.
 *
 *   S[k, v] = rnd(key_k) . rnd(query_v) / sqrt(dk)    m_k = max_v S[k, v]    E = exp(S - m)    l_k = sum_v E[k, v]
 *   out_k = (sum_v rnd(E[k, v]) rnd(value_v)) / l_k   lse_k = m_k + log l_k
 *   per window and head.  kqv, windows, num_windows, num_rows, max_num_nodes, out, lse as ptgnn_amd_block_attention_f32
 *   takes them: kqv stays fp32 in memory and is read in place; keys, queries and values are rounded to `dtype`
 *   (PTGNN_AMD_HALF_BF16 / _F16; round to nearest even with gradual underflow, as tensor.to(dtype)) on their way into
 *   LDS, the unnormalised probabilities E in registers (with the running maximum of the 32-query tile they are formed
 *   in).  Products on v_mfma_f32_32x32x16_{bf16,f16}; the scale, the mask, the running maximum and sum, exp, l (the sum
 *   of the UNROUNDED E), the division and every accumulation are fp32.  A value beyond the fp16 range rounds to inf, as
 *   tensor.half() gives.
 *   ptgnn_amd_attention16_block_supported(dk, dv, dtype): 1 when the kernel takes the widths (1 <= dk, dv <= 128 and a
 *     known dtype id), else 0; needs no device.
 * kqv must be 4-byte aligned; with a 16-byte aligned base, ld_kqv % 4 == 0, dk % 4 == 0 and dv % 4 == 0 the rows are
 * loaded as float4, else element by element -- the same values and bits either way.  Error codes as
 * ptgnn_amd_block_attention_f32, plus EINVAL for an unknown dtype id; bad arguments are refused before any HIP call.
 * Every sum runs in tile order inside one wave: no atomics, deterministic, and a window's rows do not depend on its place
 * in the batch.  (The names put "attention16" before "block": the ptgnn_amd_block_attention* prefix is a closed set of
 * four, and the ABI version stays -- the entries are additive, like every 16-bit entry before them.)
 * ---------------------------------------------------------------------------------------- */
int ptgnn_amd_attention16_block_supported(int32_t dk, int32_t dv, int dtype);
int ptgnn_amd_attention16_block(const float *kqv, int64_t ld_kqv, const int32_t *windows, int64_t num_windows,
                                int64_t num_rows, int32_t max_num_nodes, int32_t num_heads, int32_t dk, int32_t dv,
                                float *out, int64_t ld_out, float *lse, int dtype, void *stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* PTGNN_AMD_H_ */
