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
