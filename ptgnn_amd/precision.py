"""Opt-in 16-bit matrix-core inputs for the GGNN layer's dense blocks, the MLP-MP layer's message GEMMs and the
attention layer's inference forward.

The default is `torch.float32`: every dense block runs the exact-fp32 MFMA kernels, bit for bit as without this module.
With `torch.bfloat16` / `torch.float16` the INFERENCE routes of `GatedMessagePassingLayer` (and, with `training=True`,
its TRAINING routes: below) round the operands of the
table-form message Linear and of the GRU cell's gate GEMMs to that type (round to nearest even, like `tensor.to(dtype)`)
and multiply them on the 16-bit matrix cores (csrc/half_gemm.hip); accumulation, bias, gate math, the aggregation and
the stored states stay fp32.  That is what an `enable_amp` user of the reference trainer gets from autocast
(trainer.py:205,221; the reference up-casts only at the scatter, abstractmessagepassing.py:43-50).

    ptgnn_amd.set_matrix_inputs("autocast")       # next to enable_amp: follow torch.autocast on GPU tensors
    with ptgnn_amd.matrix_inputs(torch.bfloat16): # or explicitly, for a block
        out = model(batch)

The grouped per-edge GEMM of the edge form (many sparse edge types: the Graph2Class batches) has a switch of its own,
because it is the one GPU route that stayed fp32 when the setting first shipped and existing users keep their bits:

    with ptgnn_amd.matrix_inputs(torch.bfloat16, edge_gemm=True):   # also set_matrix_inputs(v, edge_gemm=True)
        out = model(batch)

With the flag the inference edge form (`GatedMessagePassingLayer._forward_fused`) rounds the gathered source states and
the per-type weights like the table form does and runs csrc/edge_gemm16.hip, in both of its launch forms (one row per
distinct (type, source) pair, or one per edge when the unique-row back-off fires) -- same bits either way.  Every call
without the keyword means `edge_gemm=False`; `set_matrix_inputs(torch.float32)` resets everything, and `edge_gemm=True`
with float32 is accepted and means fp32.

Training has a switch of its own too, for the same reason (`matrix_inputs(torch.bfloat16)` while training is pinned to
fp32 bits):

    ptgnn_amd.set_matrix_inputs("autocast", training=True)          # next to enable_amp: the training loop follows too
    with ptgnn_amd.matrix_inputs(torch.bfloat16, training=True):
        loss = model(batch); loss.backward()

With the flag the GRU cell at the end of every GGNN training route and the message Linear of the table-form training
route become 16-bit autograd nodes (ptgnn_amd/dense.py): the forward GEMMs, the input-gradient GEMMs and the
weight-gradient GEMMs (csrc/wgrad16.hip) round their operands -- activations and incoming gradients in registers, the
weights by torch -- while states, saved tensors, gradients, accumulation, bias, bias gradients (column sums of the
unrounded fp32 gradient), gate math and gate-math backward stay fp32.  fp16 overflow of a rounded gradient becomes inf,
as `tensor.half()` gives and `GradScaler` expects.  Every call without the keyword means `training=False`;
`set_matrix_inputs(torch.float32)` resets it, and `training=True` with float32 is accepted and means fp32.  The forward
of a training call under the flag has the bits of the inference route under the same setting.

The MLP-MP layer (`MlpMessagePassingLayer`, the layer of the published Typilus Graph2Class architecture) has a switch of
its own as well -- it stayed fp32 under every setting above, and existing users keep their bits:

    with ptgnn_amd.matrix_inputs(torch.bfloat16, mlp=True):         # also set_matrix_inputs(v, mlp=True)
        out = model(batch)

With the flag the layer's INFERENCE routes with single-Linear, bias-free edge transforms and no edge features (the routes
behind `_fused_ok`, and the inference branch of `_forward_pna`) round the operands of the message transformation -- the
node states and the first-Linear weights -- and multiply them on the 16-bit matrix cores: the [N, (1|2) T M] table Linear
of the table form (ptgnn_amd_half_linear on the stacked source and target halves), and the grouped per-edge GEMM of the
edge form (csrc/edge_gemm16.hip: ptgnn_amd_edge_dst_linear16 over [x[src] | x[dst]], or ptgnn_amd_edge_linear16 with
`use_target_state_as_message_input=False`).  States, messages, the aggregation, GELU, LayerNorm, the dense update and
every store stay fp32.  Every call without the keyword means `mlp=False`; `set_matrix_inputs(torch.float32)` resets it,
and `mlp=True` with float32 is accepted and means fp32.  The flag is independent of the GGNN flags: a GGNN layer under
`mlp=True` alone behaves as under the plain dtype setting.

What deliberately stays fp32 in the MLP-MP layer under `mlp=True`: the dense update Linear + Tanh (1 / (2 T) of the
table's FLOPs; in the hidden-64 edge form it has no launch of its own -- `ops.gather_update` aggregates, normalises and
updates in ONE launch, and that launch is still taken); deeper or biased edge MLPs (`_forward_deep_mlps`); edge features;
aggregation modules other than exactly `PnaMessageAggregation`; `_forward_general`; `forward_sharded`; every training
route.

The attention layer (`MultiHeadSelfAttentionMessagePassing`) has a switch of its own too -- it stayed fp32 under every
setting above, and existing users keep their bits:

    with ptgnn_amd.matrix_inputs(torch.bfloat16, attention=True):   # also set_matrix_inputs(v, attention=True)
        out = model(batch)

With the flag the layer's INFERENCE forward (nothing needs a gradient, dropout inactive) runs what autocast runs in the
16-bit type in the reference (selfattmessagepassing.py:92-122): the four Linears (head transforms, summarisation,
intermediate, output: ptgnn_amd_half_linear / ptgnn_amd_linear_add16, operands rounded, fp32 accumulation) and both
products of the block attention (csrc/block_attention16.hip: keys, queries and values rounded on their way into LDS,
the unnormalised probabilities rounded in registers).  The softmax (scale, mask, running maximum and sum -- of the
unrounded probabilities -- exp, the division), both LayerNorms, the residuals, bias, ReLU and every store stay fp32.
Every call without the keyword means `attention=False`; `set_matrix_inputs(torch.float32)` resets it, and
`attention=True` with float32 is accepted and means fp32.  The flag is independent of `edge_gemm`, `training` and
`mlp`: a GGNN or MLP-MP layer under `attention=True` alone behaves as under the plain dtype setting.  The AMP up-cast
path (16-bit states) and `target_reference != "all"` go through the same branch.  Widths the 16-bit Linear does not take
(not multiples of 32) run that Linear in fp32, silently; the attention kernel takes every dk, dv in 1..128.

What deliberately stays fp32 in the attention layer under `attention=True`: its training branch (any parameter or state
that needs a gradient, or dropout > 0 in train()), including the attention backward.

That training branch has a switch of its own -- a setting beside `set_matrix_inputs`, whose keyword list is closed; it
stayed fp32 under every setting above, and existing users keep their bits:

    ptgnn_amd.set_matrix_inputs("autocast"); ptgnn_amd.set_attention_training(True)     # next to enable_amp
    with ptgnn_amd.matrix_inputs(torch.bfloat16), ptgnn_amd.attention_training():
        loss = model(batch); loss.backward()

With the switch the training branch of `MultiHeadSelfAttentionMessagePassing` runs the block attention as a 16-bit
autograd node (`scatter.block_attention(inputs=)`): the forward is csrc/block_attention16.hip -- with dropout > 0 in
its dropout mode: the same hash mask as the fp32 kernel, applied with its fp32 scale to the unnormalised probabilities
after they were summed and BEFORE their one rounding, as autocast applies nn.Dropout before the 16-bit einsum -- and the
backward is csrc/block_attention16_backward.hip: S and dP recomputed from the rounded keys, queries, values and dOut, the
softmax backward in fp32, rnd(dS) and rnd(M o P) fed to the three gradient products from registers.  The head-transform
Linear in front of it becomes the 16-bit Linear node of `training=True` (ptgnn_amd/dense.py).  kqv, out, lse, the saved
tensors, D = sum dOut o out, every gradient in memory and every accumulation stay fp32; fp16 overflow of a rounded
gradient becomes inf, as `tensor.half()` gives and `GradScaler` expects.  The dtype comes from `set_matrix_inputs`
("autocast" included); the switch is off by default, independent of the five flags, untouched by `set_matrix_inputs`
and `matrix_inputs`, and with a float32 dtype setting it means fp32.  What stays fp32 under the plain switch: the
summarisation, intermediate and output Linears (the fused fp32 Linear + activation + dropout node), both LayerNorms, the
residuals, CPU tensors and the inference branch (which follows `attention=True` alone).

Those three Linears are a second part of that switch -- `set_attention_training(True)` keeps meaning "attention and head
transforms only", and its users keep their bits:

    ptgnn_amd.set_attention_training(True, linears=True)
    with ptgnn_amd.matrix_inputs(torch.bfloat16), ptgnn_amd.attention_training(linears=True):
        loss = model(batch); loss.backward()

With `linears=True` each of the three becomes one `dense._LinearActDropout16` node on the panel-form 16-bit Linear
(csrc/panel_linear16.hip), as autocast runs them in the reference (selfattmessagepassing.py:104-122): the forward rounds
x in the kernel and the weight by torch -- one rounding of each operand --, accumulates in fp32 and applies bias, ReLU,
the hash dropout (seeds `seed + 1 / 2 / 3` beside the attention's `seed`: no two launches share a mask) and the residual
add in fp32 in its store epilogue; the input gradient and the weight gradient (csrc/wgrad16.hip's masked form) form
g * (keep ? 1 / (1 - p) : 0) * act'(y) in fp32 in registers and round it once; the bias gradient sums the unrounded
values; no mask tensor and no masked gradient reach memory.  `attention_linear_inputs(tensor)` is what the layer reads.
Widths the kernels do not take (not multiples of 32, beyond 1024) keep the fp32 node, silently.  Still fp32 under
`linears=True`: both LayerNorms, saved tensors, every gradient in memory, CPU tensors, the inference branch and every
other user of `dense.linear_act_dropout` (the MLP-MP dense update).

The edge form of the GGNN TRAINING step -- what a Graph2Class batch takes, and every batch once the layer has per-edge
dropout (`dropout_rate > 0` in train(): the reference's Typilus configuration) -- has a switch of its own as well; it
stayed fp32 under `training=True`, and existing users keep their bits:

    ptgnn_amd.set_matrix_inputs("autocast", training=True, edge_training=True)
    with ptgnn_amd.matrix_inputs(torch.bfloat16, edge_training=True):
        loss = model(batch); loss.backward()

With the flag the edge-form training branch of `GatedMessagePassingLayer.forward` runs its autograd node
(`scatter._EdgeLinear`) with 16-bit operands in all three GEMMs: the grouped per-edge forward rounds
(keep ? x[src] * scale : 0) -- the dropout mask and its fp32 scale 1 / (1 - p) applied BEFORE the one rounding, as
autocast applies nn.Dropout before the 16-bit Linear -- against the rounded [T, M, H] weights; the input gradient rounds
the incoming gradient against the rounded transposed weights and applies mask and scale to the fp32 accumulator
(csrc/edge_gemm16.hip, the masked forms); the per-type weight gradient rounds both the incoming gradient and the
gathered, masked, scaled states (csrc/edge_wgrad16.hip, deterministic).  Saved tensors, the mask bits, grad_msg, the
[E, K] input gradient, both segment sums, d x, d W and the GRU node (which follows `training=True`, independently) stay
fp32.  Every call without the keyword means `edge_training=False`; `set_matrix_inputs(torch.float32)` resets it, and
`edge_training=True` with float32 is accepted and means fp32.  The flag is independent of the other four.  With
dropout 0 a training forward under the flag has the bits of the inference per-edge launch under `edge_gemm=True`.

What stays fp32 under every setting: without `training=True` every training route (anything that needs a gradient)
except, with `edge_training=True`, the edge-form node above;
with it still the edge-form training GEMMs (`_EdgeLinear`) unless `edge_training=True`; under every flag the
edge-feature training GEMMs (`_EdgeLinearFeat`), `_general_messages`
and `forward_sharded`, every MLP-MP training route, the attention layer's training, EGC, the attention pooling
reducers and the other reducers, the heads and the decoder; without `mlp=True` all of MLP-MP; without `attention=True`
all of the attention layer; CPU tensors in
training (the torch route rounds nothing where a gradient is needed); the edge-feature route's grouped GEMM; without
`edge_gemm=True` also the grouped per-edge GEMM of the edge form.  Shapes the 16-bit kernels do not take (widths that are not multiples of 32; for the per-edge
GEMM also fewer than 2 or more than 64 edge types) run the fp32 kernels, silently.  CPU tensors
(ptgnn_amd/torch_route.py) round the same operands with torch under the dtype setting alone -- message operands
included, so the flag changes nothing there -- and a checkpoint behaves alike on both devices; the MLP-MP layer's CPU
route rounds the node states and the message Linears' weights under `mlp=True` under the same conditions as the GPU
routes (fp32 states, nothing needs a gradient); the attention layer's CPU route rounds the Linear operands, k, q, v and
the probabilities under `attention=True` under those conditions too (the NORMALISED probabilities, as autocast does;
the kernel rounds the unnormalised ones -- either way each probability carries one rounding of the 16-bit type);
"autocast" never touches CPU tensors.

The GGNN MESSAGE ROWS have a switch of their own -- a setting beside `set_matrix_inputs`, whose keyword list is closed.
Under every setting above a message row leaves its GEMM as fp32 and the aggregation reads it as fp32; the reference's
`enable_amp` produces the messages as 16-bit tensors and up-casts them only inside `_aggregate_messages`
(abstractmessagepassing.py:43-50): one rounding of each message, then fp32 accumulation in the scatter.

    with ptgnn_amd.matrix_inputs(torch.bfloat16, edge_gemm=True), ptgnn_amd.half_messages():
        out = model(batch)                                  # also ptgnn_amd.set_half_messages(True)

With the switch the inference route of `GatedMessagePassingLayer` (`_forward_fused`) stores its messages as 16-bit rows
of the dtype setting -- the table form's [N, T M] Linear under the plain dtype setting (ptgnn_amd_linear_rows16), the
edge form's grouped per-edge GEMM under `edge_gemm=True` (both launch forms: csrc/edge_gemm16.hip, same bits per row) --
each value exactly rnd(accumulator of the 16-bit launch), and aggregates them with csrc/gather_reduce16.hip: rows
up-cast in registers, fp32 accumulation in CSR order, an fp32 aggregate for the GRU cell as before.  Half the bytes of
every message row, written and read.  `message_rows(tensor, edge_form)` is what the layer reads.  The switch is off by
default, untouched by `set_matrix_inputs` / `matrix_inputs`, independent of the five flags, and takes its dtype from the
dtype setting ("autocast" included); with float32 it means fp32 rows.  Widths the aggregation does not take (message
widths that are not multiples of 32 or beyond 256) or the 16-bit GEMM does not take keep fp32 rows, silently.  CPU
tensors (torch_route.ggnn_layer) round the messages with torch under the switch, under the same inference-only
conditions as the operands, so a checkpoint behaves alike on both devices.  Out of scope, fp32 rows under the switch:
every training route; MLP-MP (a part of the switch of its own: below); EGC and PNA; `forward_sharded`; the
edge-feature route; `_amp_forward`.

The MLP-MP MESSAGE ROWS are a second part of that switch -- `set_half_messages(True)` keeps meaning "GGNN only", and its
users keep their bits:

    with ptgnn_amd.matrix_inputs(torch.bfloat16, mlp=True), ptgnn_amd.half_messages(mlp=True):
        out = model(batch)                                  # also ptgnn_amd.set_half_messages(True, mlp=True)

With `mlp=True` on BOTH settings the inference routes of `MlpMessagePassingLayer._forward_fused` store their messages as
16-bit rows and aggregate them with csrc/gather_reduce16_epi.hip.  Table form: the [N, (1|2) T M] table leaves its
16-bit Linear as 16-bit rows (ptgnn_amd_linear_rows16), and the aggregation adds the slot's source block and the
node's destination block in fp32 before the fold.  Edge form: the grouped per-edge GEMM over [x[src] | x[dst]] (or
x[src] alone) stores rnd(accumulator) per edge (ptgnn_amd_edge_rows16_dst_linear16 / ptgnn_amd_edge_rows16_linear16).
Either way the fold, the mean, GELU and LayerNorm are fp32 inside the aggregation launch and the aggregate is fp32, as
before.  `mlp_message_rows(tensor)` is what the layer reads: the 16-bit type only for fp32 GPU states with both parts
on.  Anything either end declines (a message width that is not a multiple of 32 or beyond 256, a shape the 16-bit GEMM
does not take, unaligned states, a non-stock activation or LayerNorm) runs exactly what it runs without the switch.
Deliberately fp32 rows under the switch: the one-launch `ops.gather_update` route at hidden 64 (still taken when it
applies), `_forward_pna`, deep or biased edge MLPs, edge features, `_forward_general`, `forward_sharded`, every training
route.  CPU tensors (torch_route.mlp_layer) round each message once with torch under the same conditions (string
aggregations only) -- the edge form's values; the GPU table form rounds the two halves separately.

The SCORE-FREE GRAPH2SEQ LOSS (`GruCopyingDecoder.score_free_loss`) has a setting of its own as well -- the decoder
stayed fp32 under everything above, and existing users keep their bits.  Under `enable_amp` the reference runs the
vocabulary einsum (grucopydecoder.py:111-118) in the autocast dtype:

    ptgnn_amd.set_matrix_inputs("autocast"); ptgnn_amd.set_vocabulary_loss(True)       # next to enable_amp
    with ptgnn_amd.matrix_inputs(torch.bfloat16), ptgnn_amd.vocabulary_loss():
        loss = decoder.score_free_loss(**batch); loss.backward()

With the switch the loss node of that route (`sequence._ProjectionLoss`) runs csrc/projection_loss16.hip: the rows of the
projected states and of the (dropped-out -- the dropout is applied in fp32 before the rounding, as autocast does) embedding
table are rounded on their way into LDS, the score tiles and the two gradient products run on the 16-bit matrix cores, and
the scores themselves, the bias, the normaliser, the target pick, the score gradient, d_bias and d_extra stay unrounded
fp32; the score gradient is rounded once for d_projected and d_table.  `vocabulary_loss_inputs(tensor)` is what the decoder
reads.  Off by default, untouched by `set_matrix_inputs` / `matrix_inputs`, and with a float32 dtype setting it means
fp32.  What stays fp32 under the switch: `fused_loss`, `forward`, decoding, CPU tensors, and the first Linear (hidden ->
projected, `dense.linear`) -- the next step.

The setting is process-wide (like `ops.set_gemm_mode`); the layers read it, `ptgnn_amd.ops` never does -- its
`inputs=` keyword is explicit, because inside an autograd `Function.forward` grad mode is off and an op could not tell
inference from training.
"""
import contextlib

import torch

from ptgnn_amd._lib import PtgnnAmdError

HALF_DTYPES = (torch.bfloat16, torch.float16)
_CHOICES = (torch.float32,) + HALF_DTYPES + ("autocast",)

_setting = torch.float32
_edge_gemm = False
_training = False
_mlp = False
_attention = False
_edge_training = False
_attention_training = False
_attention_linears = False
_half_messages = False
_half_messages_mlp = False
_half_messages_training = False
_vocabulary_loss = False


def _checked(v):
    if not isinstance(v, (torch.dtype, str)) or v not in _CHOICES:
        raise PtgnnAmdError(f"matrix inputs must be torch.float32, torch.bfloat16, torch.float16 or 'autocast' (got {v!r})")
    return v


def _set(v, edge_gemm, training=False, mlp=False, attention=False, edge_training=False):
    global _setting, _edge_gemm, _training, _mlp, _attention, _edge_training
    prev = (_setting, _edge_gemm, _training, _mlp, _attention, _edge_training)
    _setting, _edge_gemm, _training, _mlp, _attention, _edge_training = \
        _checked(v), bool(edge_gemm), bool(training), bool(mlp), bool(attention), bool(edge_training)
    return prev


def set_matrix_inputs(v, *, edge_gemm=False, training=False, mlp=False, attention=False, edge_training=False):
    """Set the operand type of the GGNN inference GEMMs, whether the edge form's grouped per-edge GEMM follows it,
    whether the GGNN training routes do, whether the MLP-MP layer's inference message GEMMs do, whether the attention
    layer's inference forward does, and whether the GGNN edge-form training node does; returns the previous dtype
    setting."""
    return _set(v, edge_gemm, training, mlp, attention, edge_training)[0]


def get_matrix_inputs():
    return _setting


@contextlib.contextmanager
def matrix_inputs(v, *, edge_gemm=False, training=False, mlp=False, attention=False, edge_training=False):
    prev = _set(v, edge_gemm, training, mlp, attention, edge_training)
    try:
        yield
    finally:
        _set(*prev)


def resolve(tensor: torch.Tensor) -> torch.dtype:
    """The dtype the setting means for a layer call on `tensor`: "autocast" is the CUDA autocast dtype for a GPU tensor
    while autocast is enabled (when that is a 16-bit type), else float32."""
    v = _setting
    if v == "autocast":
        if tensor.is_cuda and torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            return dt if dt in HALF_DTYPES else torch.float32
        return torch.float32
    return v


def edge_gemm_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the edge form's grouped per-edge GEMM for a layer call on `tensor`: `resolve(tensor)` when the
    setting was made with `edge_gemm=True`, else float32."""
    return resolve(tensor) if _edge_gemm else torch.float32


def training_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the GGNN training routes' 16-bit autograd nodes for a layer call on `tensor`: `resolve(tensor)` when
    the setting was made with `training=True` and the tensor is on a GPU, else float32."""
    return resolve(tensor) if _training and tensor.is_cuda else torch.float32


def edge_training_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the GGNN edge-form training node's three GEMMs for a layer call on `tensor`: `resolve(tensor)` when
    the setting was made with `edge_training=True` and the tensor is on a GPU, else float32."""
    return resolve(tensor) if _edge_training and tensor.is_cuda else torch.float32


def mlp_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the MLP-MP layer's inference message GEMMs for a layer call on `tensor`: `resolve(tensor)` when the
    setting was made with `mlp=True`, else float32."""
    return resolve(tensor) if _mlp else torch.float32


def attention_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the attention layer's inference Linears and block attention for a layer call on `tensor`:
    `resolve(tensor)` when the setting was made with `attention=True`, else float32."""
    return resolve(tensor) if _attention else torch.float32


def set_attention_training(on, linears=False) -> bool:
    """Whether the attention layer's TRAINING branch (block attention forward with dropout, its backward, the
    head-transform Linear) takes the 16-bit type of the dtype setting -- and, with `linears=True`, whether its
    summarisation, intermediate and output Linears do too (the panel-form 16-bit Linear + activation + dropout + residual
    node); returns the previous value of the first.  A setting of its own: `set_matrix_inputs` / `matrix_inputs` neither
    read nor reset it.  Every call without the keyword means `linears=False`."""
    return _set_attention_training(on, linears)[0]


def _set_attention_training(on, linears):
    global _attention_training, _attention_linears
    prev = (_attention_training, _attention_linears)
    _attention_training, _attention_linears = bool(on), bool(on) and bool(linears)
    return prev


@contextlib.contextmanager
def attention_training(on=True, linears=False):
    prev = _set_attention_training(on, linears)
    try:
        yield
    finally:
        _set_attention_training(*prev)


def attention_training_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the attention layer's training branch for a layer call on `tensor`: `resolve(tensor)` when
    `set_attention_training` is on and the tensor is on a GPU, else float32."""
    return resolve(tensor) if _attention_training and tensor.is_cuda else torch.float32


def attention_linear_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the summarisation, intermediate and output Linears of the attention layer's training branch for a
    layer call on `tensor`: `resolve(tensor)` when `set_attention_training` is on with `linears=True` and the tensor is
    on a GPU, else float32."""
    return resolve(tensor) if _attention_training and _attention_linears and tensor.is_cuda else torch.float32


def set_vocabulary_loss(on) -> bool:
    """Whether `GruCopyingDecoder.score_free_loss` (the Graph2Seq loss with the second vocabulary Linear inside it) takes
    the 16-bit type of the dtype setting for that Linear's operands; returns the previous value.  A setting of its own:
    `set_matrix_inputs` / `matrix_inputs` neither read nor reset it."""
    global _vocabulary_loss
    prev, _vocabulary_loss = _vocabulary_loss, bool(on)
    return prev


@contextlib.contextmanager
def vocabulary_loss(on=True):
    prev = set_vocabulary_loss(on)
    try:
        yield
    finally:
        set_vocabulary_loss(prev)


def vocabulary_loss_inputs(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the score-free loss's vocabulary product for a decoder call on `tensor`: `resolve(tensor)` when
    `set_vocabulary_loss` is on and the tensor is on a GPU, else float32."""
    return resolve(tensor) if _vocabulary_loss and tensor.is_cuda else torch.float32


_wide_heads = False


def set_wide_heads(on) -> bool:
    """Whether the attention pool and the copy scores past 8 heads / decoding steps run on the matrix-core kernels of
    csrc/wide_heads.hip instead of the composed operator sequence (the multi-head attention reducer with 9 .. 64 heads;
    `GruCopyingDecoder`'s training attention for targets of 9 .. 64 steps); returns the previous value.  Off by default:
    the results differ from the composed chain by fp32 rounding.  A setting of its own: `set_matrix_inputs` /
    `matrix_inputs` neither read nor reset it.  CPU tensors, up to 8 heads and shapes outside
    `ops.wide_heads_supported` ignore it."""
    global _wide_heads
    prev, _wide_heads = _wide_heads, bool(on)
    return prev


def get_wide_heads() -> bool:
    return _wide_heads


@contextlib.contextmanager
def wide_heads(on=True):
    prev = set_wide_heads(on)
    try:
        yield
    finally:
        set_wide_heads(prev)


def set_half_messages(on, mlp=False, training=False) -> bool:
    """Whether the GGNN inference route stores its messages as 16-bit rows of the dtype setting and aggregates them with
    the 16-bit-row kernel -- with `mlp=True`, whether the MLP-MP layer's inference routes do too, and with
    `training=True`, whether the GGNN edge-form training step keeps its messages, their gradient and the per-edge input
    gradient as 16-bit rows; returns the previous value of the first.  A setting of its own: `set_matrix_inputs` /
    `matrix_inputs` neither read nor reset it.  Every call without a keyword means `mlp=False, training=False`."""
    return _set_half_messages(on, mlp, training)[0]


def _set_half_messages(on, mlp, training=False):
    global _half_messages, _half_messages_mlp, _half_messages_training
    prev = (_half_messages, _half_messages_mlp, _half_messages_training)
    _half_messages, _half_messages_mlp, _half_messages_training = \
        bool(on), bool(on) and bool(mlp), bool(on) and bool(training)
    return prev


def get_half_messages() -> bool:
    return _half_messages


def get_half_messages_mlp() -> bool:
    """Whether the switch is on with `mlp=True` (what the MLP-MP layer's CPU route reads; GPU routes read
    `mlp_message_rows`)."""
    return _half_messages and _half_messages_mlp


@contextlib.contextmanager
def half_messages(on=True, mlp=False, training=False):
    prev = _set_half_messages(on, mlp, training)
    try:
        yield
    finally:
        _set_half_messages(*prev)


def message_rows(tensor: torch.Tensor, edge_form: bool) -> torch.dtype:
    """The dtype of the GGNN message rows for a layer call on `tensor`: with `set_half_messages` on, the dtype of the
    GEMM that produces them -- `edge_gemm_inputs(tensor)` for the edge form, `resolve(tensor)` for the table form --
    else float32."""
    if not _half_messages:
        return torch.float32
    return edge_gemm_inputs(tensor) if edge_form else resolve(tensor)


def mlp_message_rows(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the MLP-MP layer's message rows for an inference call on the states `tensor`: `mlp_inputs(tensor)`
    when `set_half_messages` is on with `mlp=True`, that is a 16-bit type and the states are fp32 on a GPU; else
    float32."""
    if not (_half_messages and _half_messages_mlp) or not tensor.is_cuda or tensor.dtype != torch.float32:
        return torch.float32
    return mlp_inputs(tensor)


def training_message_rows(tensor: torch.Tensor) -> torch.dtype:
    """The dtype of the [E, .] rows of the GGNN edge-form training step (messages, their gradient, the per-edge input
    gradient) for a layer call on the states `tensor`: `edge_training_inputs(tensor)` when `set_half_messages` is on with
    `training=True`, that is a 16-bit type and the states are fp32 on a GPU; else float32."""
    if not (_half_messages and _half_messages_training) or not tensor.is_cuda or tensor.dtype != torch.float32:
        return torch.float32
    return edge_training_inputs(tensor)
