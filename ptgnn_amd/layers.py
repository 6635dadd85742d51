"""Drop-in message-passing layers: same class names, constructor keywords, forward signature,
properties and (name-mangled) parameter names as the reference's
ptgnn/neuralmodels/gnn/messagepassing/{abstractmessagepassing,gatedmessagepassing,
mlpmessagepassing,residuallayers}.py and ptgnn/neuralmodels/mlp.py -- so
``GraphNeuralNetworkModel(message_passing_layer_creator=...)`` (graphneuralnetwork.py:231,298)
accepts them unchanged and ``layer.load_state_dict(reference_layer.state_dict())`` just works.

What is different is HOW a layer runs.  Inference (`torch.no_grad()` or no input requires grad,
dropout inactive, no edge features, single-Linear edge transform) takes the fused MI355X path:

    plan  = dst-sorted CSR of ALL edge types, built once per minibatch          (csr_build.hip)
    Y     = X [W_0; ...; W_{T-1}]^T              one wide fp32-MFMA GEMM        (dense_f32.hip)
    A     = reduce_{in-edges} Y[src, type] (+ Y_dst[v, type]) (+GELU+LayerNorm) (gather_reduce.hip)
    X'    = GRUCell(A, X)  |  tanh(A W^T + b)    fp32-MFMA, fused epilogues     (dense_f32.hip)

using  Linear_t(x_src) == (X W_t^T)[src]  (a bias-free Linear commutes with the row gather) and,
for the MLP layer with target state,  W_t [x_u ; x_v] = W_t^s x_u + W_t^d x_v.

With many sparse edge types the per-node table is replaced by ONE grouped per-edge GEMM over all types
(edge_gemm.hip), picked per minibatch.

Training (grad required) runs on the same kernels: the edge form is one autograd node
(ptgnn_amd/scatter.py `edge_linear`: grouped GEMM forward, split-edge weight-gradient GEMM, input
gradient through the same grouped GEMM + HIP segment-sum) with the GGNN layer's per-edge dropout folded
in as a counter-based hash mask; the table form differentiates through `scatter.gather_reduce` (backward
= the gather-reduce kernel over a backward plan); GRU / Linear blocks are `ptgnn_amd/dense.py` nodes.

Edge features ride the grouped per-edge GEMM as a third K range of its gathered A rows (`ptgnn_amd_edge_linear_feat_f32`;
nothing of the reference's [E, H + F] message input exists in memory) -- inference and, as one autograd node
(`scatter._EdgeLinearFeat`), training; deeper edge MLPs run their first Linear the same way.  Custom aggregation modules,
per-edge dropout together with edge features, biased edge MLPs and widths that are not multiples of 32 take the general
per-edge path: torch only gathers / concatenates rows, every Linear runs on the HIP GEMM (`ptgnn_amd/dense.py`, any width)
and the aggregation on the HIP segment-reduce seam with its autograd rule.  fp16 / bf16 node states (AMP) are up-cast
to fp32 on entry and the result is cast back.  No GPU path runs on a vendor BLAS or falls back to torch.

Opt-in 16-bit matrix-core inputs (`ptgnn_amd/precision.py`, off by default): the GGNN layer's INFERENCE routes round the
operands of the table-form message Linear and of the GRU cell to bf16 / fp16 and run them on csrc/half_gemm.hip; with
`edge_gemm=True` the edge form's grouped per-edge GEMM does the same on csrc/edge_gemm16.hip.  The edge-feature route's
grouped GEMM, `forward_sharded`, every other layer and the decoder stay fp32 under every setting, and so does every
training route unless the setting was made with `training=True`: then the GRU cell at the end of every GGNN training
route and the table-form training Linear are 16-bit autograd nodes (`dense._GruCell`, `dense._Linear` with `inputs=`:
forward, input gradients and weight gradients on csrc/half_gemm.hip and csrc/wgrad16.hip); `_EdgeLinear`,
`_EdgeLinearFeat` and `_general_messages` stay fp32.  With `edge_training=True` (a flag of its own again) the edge-form
training branch of the GGNN layer runs `_EdgeLinear` with 16-bit operands: the masked per-edge forward and input
gradient on csrc/edge_gemm16.hip, the per-type weight gradient on csrc/edge_wgrad16.hip.

Device dispatch (round 5): tensors on the CPU take `ptgnn_amd/torch_route.py` (plain torch operators, so that the
reference's `predict.py` -- which restores and runs on "cpu" -- and a CPU `ModelTrainer` work with these layers);
tensors on the GPU always take the HIP library and raise when it is missing.

How to read the file: every layer's `forward` is the host / AMP preamble followed by an ORDERED list of "condition ->
route"; the order is behaviour.  Route bodies are the `_forward_*` methods of the layer (they need its name-mangled
modules).  What the layers share is spelled once at module level: `_has_edge_features`, `_first_linear_gemm_ok` (when
the first Linear of every edge MLP can be the grouped GEMM), `_edge_mlp_tail` (the rest of the edge MLPs),
`_train_edge_messages` (training, edge form) and the `_shard_*` table plumbing of `forward_sharded`; the MLP layer's
`_epilogue` decides once whether GELU + LayerNorm fold into a launch.
"""
import contextlib
import os
import threading
import weakref
from typing import Dict, List, Optional, Tuple, Union

import torch
from torch import nn

from ptgnn_amd import _lib, dense, ops, precision, torch_route
from ptgnn_amd.scatter import (block_attention as block_attention_autograd, edge_linear as edge_linear_autograd,
                               edge_linear_feat as edge_linear_feat_autograd,
                               gather_reduce as gather_reduce_autograd, graph_norm as graph_norm_autograd,
                               pna_aggregate as pna_aggregate_autograd, scatter_mean, segment_reduce)

try:  # inside a ptgnn install the layers ARE ptgnn layers
    from ptgnn.neuralmodels.gnn.messagepassing.abstractmessagepassing import (  # type: ignore
        AbstractMessageAggregation, AbstractMessagePassingLayer)
except Exception:  # standalone (e.g. the GPU box): identical interface
    class AbstractMessagePassingLayer(nn.Module):
        """Interface of abstractmessagepassing.py:8-60."""

        def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                    reference_node_graph_idx, edge_features) -> torch.Tensor:
            raise NotImplementedError

        def _aggregate_messages(self, messages, message_targets, num_nodes, aggregation_fn: str):
            from ptgnn_amd.scatter import scatter
            msg_dtype = messages.dtype
            return scatter(messages.to(torch.float32), index=message_targets, dim=0,
                           dim_size=num_nodes, reduce=aggregation_fn).to(msg_dtype)

        @property
        def input_state_dimension(self) -> int:
            raise NotImplementedError

        @property
        def output_state_dimension(self) -> int:
            raise NotImplementedError

    class AbstractMessageAggregation(nn.Module):
        def forward(self, messages, message_targets, num_nodes):
            raise NotImplementedError

        def output_state_size(self, message_input_size: int) -> int:
            raise NotImplementedError

Adj = List[Tuple[torch.Tensor, torch.Tensor]]


# Tensors derived from parameters that may be shared by the layer calls of ONE forward pass (e.g. the
# stacked per-type weights of a tied GGNN layer that the Typilus stack applies seven times): inside a
# `forward_scope()` -- ptgnn_amd.gnn.GraphNeuralNetwork opens one around its layer loop -- they are built
# once, so autograd accumulates one stacked gradient per use instead of T small ones.  Outside a scope
# nothing is cached (the autograd graph of a cached tensor must not outlive its forward).
_SCOPE = threading.local()


@contextlib.contextmanager
def forward_scope():
    outer = getattr(_SCOPE, "cache", None)
    if outer is None:
        _SCOPE.cache = {}
        from ptgnn_amd import dense
        dense.clear_transposed_cache()   # W^T copies of the previous backward: valid for one forward / backward pair
    try:
        yield
    finally:
        _SCOPE.cache = outer


def _scoped(owner, name, make):
    """Per-thread cache keyed on the module OBJECT (kept alive by the key, so an id() can never be reused
    by another module while the entry exists)."""
    cache = getattr(_SCOPE, "cache", None)
    if cache is None or not torch.is_grad_enabled():
        return make()
    key = (owner, name)
    val = cache.get(key)
    if val is None:
        val = cache[key] = make()
    return val


# Output hint: ptgnn_amd.gnn.GraphNeuralNetwork knows which layer feeds a ConcatResidualLayer; it hands that layer the
# right half of the [N, D0 + D1] buffer the residual will return, so the layer's last kernel writes there and the
# residual only has to fill in the left half instead of torch.cat-ing both (inference only; a layer is free to
# ignore the hint -- the residual checks what it actually got).
def set_output_hint(buf: Optional[torch.Tensor]) -> None:
    _SCOPE.out_hint = buf


def _take_output_hint(rows: int, cols: int, like: torch.Tensor, vector_stores: bool = False) -> Optional[torch.Tensor]:
    hint = getattr(_SCOPE, "out_hint", None)
    _SCOPE.out_hint = None
    if hint is None or torch.is_grad_enabled() and like.requires_grad:
        return None
    if tuple(hint.shape) != (rows, cols) or hint.dtype != torch.float32 or hint.device != like.device:
        return None
    if vector_stores and (hint.data_ptr() % 16 != 0 or (rows > 1 and hint.stride(0) % 4 != 0) or hint.stride(1) != 1):
        return None
    return hint


def _no_grad_needed(*tensors) -> bool:
    if not torch.is_grad_enabled():
        return True
    return not any(t is not None and t.requires_grad for t in tensors)


# Per-edge grouped GEMM vs per-node pre-transform: FLOPs are 2*E*K*M vs 2*N*T*K*M, the per-edge rows pay a
# random 512-B gather each; measured crossover on MI355X (profiles/) is near E ~ 0.8 * N * T.
EDGE_PATH_BIAS = 1.25
# GGNN inference, edge form: one message row per distinct (edge type, source) pair instead of one per edge
UNIQUE_MESSAGES = os.environ.get("PTGNN_AMD_UNIQUE_MESSAGES", "1") not in ("", "0")


def _prefer_edge_path(num_edges: int, num_nodes: int, num_types: int, state_dim: int, msg_dim: int) -> bool:
    if state_dim % 32 != 0 or msg_dim % 4 != 0 or num_types < 2:
        return False
    return num_edges * EDGE_PATH_BIAS < num_nodes * num_types


def _has_edge_features(feature_dim: int, edge_features) -> bool:
    """Whether a layer call carries per-edge features: the layer was built for them, or a non-empty tensor came in."""
    return feature_dim != 0 or any(f is not None and f.shape[-1] != 0 for f in edge_features)


def _stack_detached(weights) -> torch.Tensor:
    """[T*M, H] = [W_0; ...; W_{T-1}] without gradient, rebuilt per call: a cache keyed on parameter versions would go
    stale under `p.data` updates (EMA, weight clipping), and the copy is tiny next to the GEMM."""
    return weights[0].detach() if len(weights) == 1 else torch.cat([w.detach() for w in weights], dim=0)


def _kernel_act(act: Optional[nn.Module]) -> Optional[str]:
    """The kernels' name of a dense activation module; None without one and for modules the kernels do not fuse."""
    return "tanh" if isinstance(act, nn.Tanh) else ("relu" if isinstance(act, nn.ReLU) else None)


def _edge_messages(table: torch.Tensor, adjacency_lists, plan, weights, inputs=None, rounded=None):
    """GGNN messages of the edge form (inference) and the `col` that maps CSR slots to their rows: one row per distinct
    (edge type, source) pair of the plan where the shared-row launch applies (GraphPlan.unique_messages), else one row
    per edge in reference order (gatedmessagepassing.py:50-61).  The aggregate has the same bits either way -- also
    under 16-bit `inputs` (with `rounded`, the [T, M, H] stack of the rounded weights), which both launches follow."""
    if UNIQUE_MESSAGES and ops.edge_linear_shared_supported(table.shape[1], weights[0].shape[0], len(weights)):
        uniq = plan.unique_messages()
        if uniq is not None:
            return ops.edge_linear_shared(table, uniq, weights, inputs=inputs, rounded=rounded), uniq.slot_row
    return ops.edge_linear(table, adjacency_lists, weights, False, inputs=inputs, rounded=rounded), plan.perm


def _feat_gemm_ok(node_states, edge_features, state_dim: int, out_dim: int, *params, shapes_only: bool = False) -> bool:
    """Inference with per-edge features (graphneuralnetwork.py:162-186 -> gatedmessagepassing.py:57-61 /
    mlpmessagepassing.py:96-98): the grouped per-edge GEMM reads the feature rows as a third K range of its A operand
    (ptgnn_amd_edge_linear_feat_f32), so the reference's [E, H (+H) + F] input matrix is never built."""
    if node_states.dtype != torch.float32 or state_dim % 32 != 0 or out_dim % 4 != 0:
        return False
    if any(f is None or f.shape[-1] == 0 or f.device != node_states.device or f.dtype != torch.float32
           for f in edge_features):
        return False   # float64 / integer / other-device features: the general path (torch.cat promotes like the reference)
    if len({int(f.shape[-1]) for f in edge_features}) != 1:
        return False
    if shapes_only:     # the caller has a differentiable form (scatter.edge_linear_feat): gradients are no obstacle
        return True
    return (not torch.is_grad_enabled()) or _no_grad_needed(node_states, *edge_features, *params)


def _edge_training_ok(state_dim: int, msg_dim: int) -> bool:
    """The grouped edge GEMM needs its reduction width % 32 == 0: the state width in the forward, the
    message width in the input-gradient GEMM."""
    return state_dim % 32 == 0 and msg_dim % 32 == 0


def _dropout_seed() -> int:
    """A fresh 62-bit seed for the hash dropout mask, drawn from torch's CPU generator (so
    torch.manual_seed makes training runs repeatable) without touching the device."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _train_edge_messages(owner, x, plan, weights, use_dst: bool, p: float = 0.0, seed_xor: int = 0, key: str = "edge_w",
                         inputs=None):
    """Training, edge form: the grouped per-edge GEMM as one autograd node (forward + both gradients on HIP) over the
    per-type weights stacked once per forward scope, with the reference's per-edge input dropout folded in as a hash
    mask (one seed draw per call with p > 0; `seed_xor` tells the ranks of a sharded graph apart).  `inputs`: the 16-bit
    operand type of the node's three GEMMs (precision.edge_training_inputs; None / float32: the fp32 node)."""
    w_stack = _scoped(owner, key, lambda: torch.stack(weights))
    return edge_linear_autograd(x, plan, w_stack, use_dst, p, (_dropout_seed() ^ seed_xor) if p > 0 else 0,
                                inputs=inputs)


_AMP_DTYPES = (torch.float16, torch.bfloat16)


def _half_weights(owner, name: str, dtype, kind: int, k_or_m: int, n_out_or_hd: int, make):
    """The rounded copies of a layer's weights for a 16-bit matrix-input setting (ptgnn_amd/precision.py), made by torch
    (`w.detach().to(dtype).contiguous()`) once per forward scope; None under float32 and for shapes the 16-bit kernels
    do not take (the op then runs its fp32 kernel)."""
    if dtype == torch.float32 or not ops.half_supported(kind, k_or_m, n_out_or_hd, dtype):
        return None
    return _scoped(owner, (name, dtype), make)


def _amp_forward(layer, node_states, adjacency_lists, edge_features, cast_features: bool = True) -> torch.Tensor:
    """AMP (trainer.py:205,221): the reference computes messages in the autocast dtype and up-casts them to fp32 at the
    aggregation (abstractmessagepassing.py:43-50).  Here the whole layer runs in fp32 on the HIP kernels -- every
    intermediate at least as precise as the reference's -- and only the returned states go back to the caller's dtype.
    Under a 16-bit matrix-input setting (ptgnn_amd/precision.py) the up-cast states take the GGNN layer's 16-bit routes
    like any fp32 states: rounding an up-cast value is exact."""
    if cast_features:
        edge_features = [f.float() if f is not None and f.dtype in _AMP_DTYPES else f for f in edge_features]
    return layer.forward(node_states.float(), adjacency_lists, None, None, None, edge_features).to(node_states.dtype)


def _overlap_reduces():
    from ptgnn_amd import sharded
    return sharded.OVERLAP_REDUCES


def _run_mlp(mlp: "MLP", x: torch.Tensor) -> torch.Tensor:
    """ptgnn/neuralmodels/mlp.py:79-80 with every nn.Linear on the HIP GEMM (general per-edge path)."""
    for m in mlp.modules_in_order:
        x = dense.linear(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
    return x


def _first_linear_gemm_ok(mlps, training: bool, state_dim: int, differentiable: bool) -> bool:
    """Whether the FIRST Linear of every edge MLP can run as the grouped per-edge GEMM: bias-free, and no active Dropout
    inside the edge MLPs (the GEMM gathers its input rows itself).  `differentiable`: the route may need the autograd
    form (`_EdgeLinear` / `_EdgeLinearFeat`), which also wants one weight shape for all types and the widths of
    `_edge_training_ok`; the inference-only route with edge features asks for neither."""
    first = [m.linears[0] for m in mlps]
    if any(l.bias is not None for l in first):
        return False
    if training and any(isinstance(m, nn.Dropout) and m.p > 0 for e in mlps for m in e.modules_in_order):
        return False
    if not differentiable:
        return True
    return len({tuple(l.weight.shape) for l in first}) == 1 and _edge_training_ok(state_dim, first[0].weight.shape[0])


def _edge_mlp_tail(mlps, adjacency_lists, hid: torch.Tensor, differentiable: bool, single_block_as_is: bool = False):
    """The modules after the first Linear of every edge MLP, run on the type's [E_t, hidden] block of rows of `hid` (the
    first Linear's output for all edges, type-major); returns the [E, M] messages.  Differentiable form: HIP Linear
    autograd nodes, the blocks concatenated (`single_block_as_is`: one type's block is returned without the copy).
    Inference form: the type's last Linear writes its block of a preallocated message matrix in place, no concat."""
    messages = None
    if not differentiable:
        messages = torch.empty(hid.shape[0], mlps[0].linears[-1].out_features, dtype=torch.float32, device=hid.device)
    outs, off = [], 0
    for (src, _), edge_mlp in zip(adjacency_lists, mlps):
        n = int(src.shape[0])
        mods = edge_mlp.modules_in_order
        rest = mods[next(i for i, m in enumerate(mods) if isinstance(m, nn.Linear)) + 1:]
        h = hid[off:off + n]
        last = max((i for i, m in enumerate(rest) if isinstance(m, nn.Linear)), default=-1)
        for i, m in enumerate(rest):
            if not isinstance(m, nn.Linear):
                h = m(h)
            elif differentiable:
                h = dense.linear(h, m.weight, m.bias)
            else:
                h = ops.linear(h, m.weight, m.bias, out=messages[off:off + n] if i == last and n > 0 else None)
        if differentiable:
            outs.append(h)
        elif last < 0 and n > 0:
            messages[off:off + n].copy_(h)
        off += n
    if not differentiable:
        return messages
    return outs[0] if single_block_as_is and len(outs) == 1 else torch.cat(outs, dim=0)


# Table plumbing of the sharded layers (ptgnn_amd/sharded.py).  `w` is the stacked source weight [T*M, H]; what travels
# in the table form is decided by its shape: message-table rows when T*M <= H (no wider than the state, and no
# duplicated GEMM work), else node states, pre-transformed after arrival (the weights are replicated).
def _shard_source_table(shard, node_states: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Single-block table form, inference: the message table of this rank's [own | halo] rows."""
    if w.shape[0] <= w.shape[1]:
        y = shard.new_table(w.shape[0], node_states)
        ops.linear(node_states, w, out=y[: shard.n_local])
        shard.exchange_into(y)
        return y
    return ops.linear(shard.exchange(node_states), w)


def _shard_source_table_autograd(shard, node_states: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The differentiable twin of `_shard_source_table` (backward = transposed all-to-all + HIP segment-sum)."""
    if w.shape[0] <= w.shape[1]:
        return shard.exchange_autograd(dense.linear(node_states, w))
    return dense.linear(shard.exchange_autograd(node_states), w)


def _shard_two_blocks(shard, node_states: torch.Tensor, w: Optional[torch.Tensor], edge_messages=None):
    """Two-block mode (the own-source block aggregates while the halo rows travel): the `(work, table_of)` pair of
    `sharded.aggregate_two_blocks`.  Edge form: `edge_messages(table, adjacency_lists, plan) -> (messages, col)` makes a
    block's messages from the local table [own | halo], and `w` is not read; table form: `edge_messages` is None."""
    n, H = shard.n_local, node_states.shape[1]
    if edge_messages is not None or w.shape[0] > H:      # node states travel
        table = shard.new_table(H, node_states)
        table[:n].copy_(node_states)
        work = shard.begin_exchange(table)
        if edge_messages is not None:
            def table_of(block):
                adj, plan = (shard.adj_own, shard.plan_own) if block == "own" else (shard.adj_halo, shard.plan_halo)
                return edge_messages(table, adj, plan) + (0,)
            return work, table_of
        y = shard.new_table(w.shape[0], node_states)
        ops.linear(node_states, w, out=y[:n])

        def table_of(block):
            if block == "halo":
                ops.linear(table[n:], w, out=y[n:])
            return y, None, None
        return work, table_of
    y = shard.new_table(w.shape[0], node_states)         # message-table rows travel
    ops.linear(node_states, w, out=y[:n])
    return shard.begin_exchange(y), lambda block: (y, None, None)


def _check_device(node_states: torch.Tensor):
    """The sharded forms (RCCL halo exchange) exist on the GPU only."""
    if not node_states.is_cuda:
        raise _lib.PtgnnAmdError(
            "forward_sharded runs on the MI355X only; node_states is on "
            f"{node_states.device}. (The unsharded `forward` takes CPU tensors through ptgnn_amd.torch_route.)")


def _on_host(node_states: torch.Tensor) -> bool:
    """Device dispatch of the unsharded layers, like a torch operator's: CPU tensors take the plain-torch route
    (ptgnn_amd/torch_route.py: the reference's own `predict.py` restores and runs a model on "cpu",
    typilus/predict.py:25-27; trainer.py:392-395 trains there without a GPU); GPU tensors ALWAYS take
    libptgnn_amd.so and raise when it is missing or fails -- there is no way from a GPU tensor into the torch route."""
    return not node_states.is_cuda


# The node -> graph map of a minibatch, shared by GraphNorm and the global-exchange layers of ptgnn_amd/reduceops.py
_NUM_SAMPLES = []   # (weakref(index), version, max + 1) of the most recent index tensors


def _num_samples(index: torch.Tensor) -> int:
    """`index.max() + 1` -- the reference's own host read-back (globalgraphexchange.py:40, once per LAYER there);
    made once per index tensor, i.e. once per minibatch, here."""
    for ref, ver, upper in _NUM_SAMPLES:
        if ref() is index and ver == index._version:
            return upper
    upper = int(index.max()) + 1 if index.numel() else 0
    _NUM_SAMPLES.insert(0, (weakref.ref(index), index._version, upper))
    del _NUM_SAMPLES[4:]
    return upper


def _index_plan(index: torch.Tensor, num_samples: int) -> "ops.GraphPlan":
    """Plan of an element -> sample map.  The reference's reducers are plain torch_scatter calls
    (varsizedsummary.py:35-41,76-81) and accept ANY map, so every map takes the stable plan build -- cached per index
    tensor (`ops.plan_for`), i.e. once per minibatch for all global-exchange layers.  Round 2 tested the map for
    sortedness first to skip the sort for `node_to_graph_idx` (graphneuralnetwork.py:418-423,440-443); that test was
    a host read-back per minibatch, which now costs more than the ~40 us of device time the sort takes."""
    return ops.plan_for([(index, index)], int(num_samples))


# ------------------------------------------------------------------------------------------------
# MLP (ptgnn/neuralmodels/mlp.py) -- same Sequential index layout => same state_dict keys
# ------------------------------------------------------------------------------------------------
class MLP(nn.Module):
    def __init__(self, input_dimension: int, output_dimension: int,
                 hidden_layers: Union[List[int], int] = 1, use_biases: bool = False,
                 activation: Optional[nn.Module] = nn.ReLU(), dropout_rate: float = 0.0):
        super().__init__()
        if isinstance(hidden_layers, int):
            width = 32 if output_dimension == 1 else output_dimension  # mlp.py:34-43
            sizes = [width] * hidden_layers
        else:
            sizes = list(hidden_layers)
        if len(sizes) > 1:
            assert activation is not None, "Multiple linear layers without an activation"
        mods: List[nn.Module] = []
        d = input_dimension
        for h in sizes:                       # hidden block: Dropout, Linear, (activation)
            lin = nn.Linear(d, h, bias=use_biases)
            nn.init.xavier_uniform_(lin.weight)
            mods += [nn.Dropout(p=dropout_rate), lin] + ([activation] if activation is not None else [])
            d = h
        out = nn.Linear(d, output_dimension, bias=use_biases)   # output block: Dropout, Linear
        nn.init.xavier_uniform_(out.weight)
        mods += [nn.Dropout(p=dropout_rate), out]
        self.__mlp_modules = nn.Sequential(*mods)

    @property
    def linears(self) -> List[nn.Linear]:
        return [m for m in self.__mlp_modules if isinstance(m, nn.Linear)]

    @property
    def modules_in_order(self) -> List[nn.Module]:
        return list(self.__mlp_modules)

    @property
    def is_single_linear(self) -> bool:
        ls = self.linears
        return len(ls) == 1 and ls[0].bias is None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.__mlp_modules(x)


# ------------------------------------------------------------------------------------------------
# GGNN layer
# ------------------------------------------------------------------------------------------------
class GatedMessagePassingLayer(AbstractMessagePassingLayer):
    """GGNN layer; constructor and semantics of gatedmessagepassing.py:8-77."""

    def __init__(self, state_dimension: int, message_dimension: int, num_edge_types: int,
                 message_aggregation_function: str, dropout_rate: float = 0.0,
                 edge_feature_dimension: int = 0):
        super().__init__()
        self.__edge_message_transformation_layers = nn.ModuleList(
            [nn.Linear(state_dimension + edge_feature_dimension, message_dimension, bias=False)
             for _ in range(num_edge_types)])
        for lin in self.__edge_message_transformation_layers:
            nn.init.xavier_normal_(lin.weight, gain=(1 / num_edge_types) ** 0.5)
        self.__state_update = nn.GRUCell(input_size=message_dimension, hidden_size=state_dimension)
        nn.init.orthogonal_(self.__state_update.weight_hh)
        nn.init.xavier_uniform_(self.__state_update.weight_ih)
        nn.init.normal_(self.__state_update.bias_hh, std=1e-5)
        nn.init.normal_(self.__state_update.bias_ih, std=1e-5)
        self.__state_dimension = state_dimension
        self.__aggregation_fn = message_aggregation_function
        self.__dropout = nn.Dropout(p=dropout_rate)
        self._message_dimension = message_dimension
        self._edge_feature_dimension = edge_feature_dimension

    # -- fused path -------------------------------------------------------------------------
    def _stacked_edge_weights(self) -> torch.Tensor:
        """[T*M, H] = [W_0; ...; W_{T-1}], detached (see `_stack_detached`)."""
        return _stack_detached([lin.weight for lin in self.__edge_message_transformation_layers])

    def _table_ok(self, node_states, edge_features) -> bool:
        """Message == row of the per-node table X [W_0; ...]^T: no edge features, no per-edge dropout."""
        if _has_edge_features(self._edge_feature_dimension, edge_features):
            return False
        if self.training and self.__dropout.p > 0:
            return False
        if self.__aggregation_fn not in ops.REDUCE_IDS:   # "mul": the scatter seam's own kernel (general path)
            return False
        return node_states.dtype == torch.float32

    def _fused_ok(self, node_states, edge_features) -> bool:
        if not self._table_ok(node_states, edge_features):
            return False
        return (not torch.is_grad_enabled()) or _no_grad_needed(node_states, *self.parameters())

    def forward(self, node_states: torch.Tensor, adjacency_lists: Adj, node_to_graph_idx,
                reference_node_ids: Dict[str, torch.Tensor],
                reference_node_graph_idx: Dict[str, torch.Tensor],
                edge_features: List[torch.Tensor]) -> torch.Tensor:
        assert len(adjacency_lists) == len(self.__edge_message_transformation_layers)
        if _on_host(node_states):
            return torch_route.ggnn_layer(node_states, adjacency_lists, edge_features,
                                          list(self.__edge_message_transformation_layers), self.__dropout,
                                          self.__state_update, self.__aggregation_fn,
                                          inputs=self._host_matrix_inputs(node_states, edge_features))
        if node_states.dtype in _AMP_DTYPES:
            return _amp_forward(self, node_states, adjacency_lists, edge_features)
        num_nodes, H, M = node_states.shape[0], self.__state_dimension, self._message_dimension
        plan = ops.plan_for(adjacency_lists, num_nodes)
        if self._fused_ok(node_states, edge_features):
            return self._forward_fused(node_states, adjacency_lists, plan)

        agg_fn = self.__aggregation_fn
        has_feats = _has_edge_features(self._edge_feature_dimension, edge_features)
        p = self.__dropout.p if self.training else 0.0
        ws = [l.weight for l in self.__edge_message_transformation_layers]
        train_inputs = precision.training_inputs(node_states)   # float32 unless the setting was made with training=True
        if (not has_feats and node_states.dtype == torch.float32 and _edge_training_ok(H, M)
                and (p > 0 or _prefer_edge_path(plan.num_edges, num_nodes, len(ws), H, M))):
            # training, edge form: grouped per-edge GEMM with the reference's per-edge input dropout
            # folded in (forward + both gradients on HIP), HIP segment reduce, torch GRU cell.  The node's three GEMMs
            # take 16-bit operands when the matrix-input setting was made with edge_training=True.
            agg = segment_reduce(_train_edge_messages(self, node_states, plan, ws, False, p,
                                                      inputs=precision.edge_training_inputs(node_states)),
                                 plan, agg_fn)
        elif self._table_ok(node_states, edge_features):
            # training without per-edge dropout, few edge types: differentiable HIP GEMM nodes (ptgnn_amd/dense.py)
            # for the dense blocks, the HIP kernel (forward + backward) for the aggregation
            agg = gather_reduce_autograd(dense.linear(node_states, torch.cat(ws, dim=0), inputs=train_inputs), None, plan,
                                         M, agg_fn)
        elif (has_feats and p == 0.0 and agg_fn in ops.REDUCE_IDS
                and _feat_gemm_ok(node_states, edge_features, H, M, *self.parameters())):
            return self._forward_features_inference(node_states, adjacency_lists, plan, edge_features)
        elif (has_feats and p == 0.0 and agg_fn in ops.REDUCE_IDS and _edge_training_ok(H, M)
                and _feat_gemm_ok(node_states, edge_features, H, M, shapes_only=True)):
            # training with edge features: the same grouped GEMM as one autograd node (scatter._EdgeLinearFeat) -- no
            # index_select, no [E, H + F] concat; weight / feature / state gradients on the HIP kernels
            agg = segment_reduce(edge_linear_feat_autograd(node_states, plan, ws, False, edge_features), plan, agg_fn)
        else:
            agg = segment_reduce(self._general_messages(node_states, adjacency_lists, edge_features), plan, agg_fn)
        return dense.gru_cell(self.__state_update, agg, node_states, inputs=train_inputs)

    def _host_matrix_inputs(self, node_states, edge_features):
        """The matrix-input setting as the CPU route applies it: fp32 states, inference only (as on the GPU)."""
        if node_states.dtype != torch.float32 or (self.training and self.__dropout.p > 0):
            return torch.float32
        if torch.is_grad_enabled() and not _no_grad_needed(node_states, *self.parameters(),
                                                           *[f for f in edge_features if f is not None]):
            return torch.float32
        return precision.resolve(node_states)

    def _rounded_gru_weights(self, dtype):
        gru = self.__state_update
        return _half_weights(self, "gru_w16", dtype, ops.HALF_KIND_GRU, self._message_dimension, self.__state_dimension,
                             lambda: (gru.weight_ih.detach().to(dtype).contiguous(),
                                      gru.weight_hh.detach().to(dtype).contiguous()))

    def _forward_fused(self, node_states, adjacency_lists, plan) -> torch.Tensor:
        """Inference: message table (or edge form) -> aggregation -> GRU cell, pipelined over destination-row ranges on
        large minibatches (ops.aggregate_gru).  Under a 16-bit matrix-input setting the table Linear and the GRU cell
        take the 16-bit kernels; the grouped per-edge GEMM of the edge form does when the setting was made with
        `edge_gemm=True` (both of its launch forms, so the back-off between them never changes the numerics)."""
        num_nodes, H, M = node_states.shape[0], self.__state_dimension, self._message_dimension
        gru = self.__state_update
        inputs = precision.resolve(node_states)
        if _prefer_edge_path(plan.num_edges, num_nodes, len(adjacency_lists), H, M):
            # many sparse edge types: one grouped per-edge GEMM.  The message W_t x[src] is the same row for
            # every edge of type t that leaves src: the GEMM produces one row per distinct (type, source) pair
            # of the plan (GraphPlan.unique_messages, built once per minibatch on the device) and the
            # aggregation reads it per edge -- same bits, fewer rows.
            weights = [l.weight for l in self.__edge_message_transformation_layers]
            edge_inputs = precision.edge_gemm_inputs(node_states)
            w16 = None
            if edge_inputs != torch.float32 and ops.edge_linear16_supported(H, M, len(weights), edge_inputs):
                w16 = _scoped(self, ("edge_stack16", edge_inputs),
                              lambda: torch.stack([w.detach() for w in weights]).to(edge_inputs))
            msgs, col = _edge_messages(node_states, adjacency_lists, plan, weights, inputs=edge_inputs, rounded=w16)
            tb = 0
        else:
            w = self._stacked_edge_weights()
            w16 = _half_weights(self, "edge_w16", inputs, ops.HALF_KIND_LINEAR, H, w.shape[0],
                                lambda: w.to(inputs).contiguous())
            msgs, col, tb = ops.linear(node_states, w, inputs=inputs, rounded=w16), None, None      # [N, T*M]
        return ops.aggregate_gru(msgs, plan, M, self.__aggregation_fn, node_states, gru.weight_ih, gru.weight_hh,
                                 gru.bias_ih, gru.bias_hh, type_bits=tb, col=col,
                                 out=_take_output_hint(num_nodes, H, node_states), inputs=inputs,
                                 rounded=self._rounded_gru_weights(inputs))

    def _forward_features_inference(self, node_states, adjacency_lists, plan, edge_features) -> torch.Tensor:
        """Inference with edge features: fused gather of [x[src] | features] inside the grouped GEMM (fp32 under every
        matrix-input setting; the GRU cell follows the setting)."""
        gru = self.__state_update
        inputs = precision.resolve(node_states)
        msgs = ops.edge_linear(node_states, adjacency_lists,
                               [l.weight for l in self.__edge_message_transformation_layers], False,
                               edge_feats=edge_features)
        agg = ops.gather_reduce(msgs, plan, self._message_dimension, self.__aggregation_fn, type_bits=0, col=plan.perm)
        return ops.gru_cell(agg, node_states, gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh, inputs=inputs,
                            rounded=self._rounded_gru_weights(inputs))

    def _general_messages(self, node_states, adjacency_lists, edge_features) -> torch.Tensor:
        """General per-edge path (per-edge dropout with edge features, odd widths): message order = type-major."""
        all_messages = []
        for (src, _), feats, lin in zip(adjacency_lists, edge_features,
                                        self.__edge_message_transformation_layers):
            inp = node_states.index_select(0, src)
            if feats is not None and feats.shape[-1] > 0:
                inp = torch.cat([inp, feats.to(inp.dtype)], dim=-1)
            all_messages.append(dense.linear(self.__dropout(inp), lin.weight))     # HIP GEMM, K = H + F
        return torch.cat(all_messages, dim=0)

    def forward_sharded(self, node_states: torch.Tensor, shard) -> torch.Tensor:
        """One layer over a dst-range shard (ptgnn_amd/sharded.py): `node_states` are this rank's rows; one
        all-to-all of halo rows, then the same kernels as `forward`.  Form per minibatch, like `forward`:
          * edge form (many sparse edge types, or training with per-edge dropout): the grouped per-edge GEMM
            gathers its A rows from the local table [own | halo] through the remapped adjacency lists;
          * table form: per-node pre-transform; the rows that travel are message-table rows when T*M <= H,
            else node states (pre-transformed after arrival: the weights are replicated)."""
        _check_device(node_states)
        feats = [None] * len(shard.local_adj)
        T = len(shard.local_adj)
        assert T == len(self.__edge_message_transformation_layers)
        if self._edge_feature_dimension != 0 or node_states.dtype != torch.float32:
            raise _lib.PtgnnAmdError("forward_sharded: edge features / non-fp32 states are not supported on a "
                                     "sharded graph")
        agg_fn = self.__aggregation_fn
        if agg_fn not in ops.REDUCE_IDS:
            raise _lib.PtgnnAmdError(f"forward_sharded: aggregation {agg_fn!r} is not supported on a "
                                     "sharded graph (sum / mean / max / min are)")
        M, H = self._message_dimension, self.__state_dimension
        gru = self.__state_update
        p = self.__dropout.p if self.training else 0.0
        ws = [l.weight for l in self.__edge_message_transformation_layers]
        edge_form = _prefer_edge_path(*shard.form_sizes(T * M > H), T, H, M)   # one decision for the whole group
        if not self._fused_ok(node_states, feats):
            # training.  Edge form: differentiable halo exchange (backward = transposed all-to-all + HIP
            # segment-sum) -> grouped per-edge GEMM node with the hash dropout folded in -> HIP segment reduce
            if _edge_training_ok(H, M) and (p > 0 or edge_form):
                msgs = _train_edge_messages(self, shard.exchange_autograd(node_states), shard.plan, ws, False, p,
                                            seed_xor=0x9E3779B97F4A7C15 * (shard.rank + 1) & (2 ** 62 - 1))
                agg = segment_reduce(msgs, shard.plan, agg_fn)
            elif p > 0:
                raise _lib.PtgnnAmdError("forward_sharded: per-edge dropout needs state and message widths that "
                                         "are multiples of 32")
            else:
                y = _shard_source_table_autograd(shard, node_states, torch.cat(ws, dim=0))
                agg = gather_reduce_autograd(y, None, shard.plan, M, agg_fn)
            return dense.gru_cell(gru, agg, node_states)

        def edge_messages(table, adj, plan):
            return _edge_messages(table, adj, plan, ws)
        if shard.overlap and agg_fn in _overlap_reduces():
            from ptgnn_amd import sharded
            work, table_of = _shard_two_blocks(shard, node_states, None if edge_form else self._stacked_edge_weights(),
                                               edge_messages if edge_form else None)
            agg = sharded.aggregate_two_blocks(shard, work, table_of, M, agg_fn)
        elif edge_form:
            msgs, col = edge_messages(shard.exchange(node_states), shard.local_adj, shard.plan)
            agg = ops.gather_reduce(msgs, shard.plan, M, agg_fn, type_bits=0, col=col)
        else:
            y = _shard_source_table(shard, node_states, self._stacked_edge_weights())
            agg = ops.gather_reduce(y, shard.plan, M, agg_fn)
        return ops.gru_cell(agg, node_states, gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh)

    @property
    def input_state_dimension(self) -> int:
        return self.__state_dimension

    @property
    def output_state_dimension(self) -> int:
        return self.__state_dimension

    def export_weights(self) -> Dict:
        """Weights in the layout the parity oracle consumes (tests only read this)."""
        gru = self.__state_update
        return {"kind": "ggnn",
                "edge_w": [l.weight.detach().cpu() for l in self.__edge_message_transformation_layers],
                "w_ih": gru.weight_ih.detach().cpu(), "w_hh": gru.weight_hh.detach().cpu(),
                "b_ih": gru.bias_ih.detach().cpu(), "b_hh": gru.bias_hh.detach().cpu(),
                "agg": self.__aggregation_fn}


# ------------------------------------------------------------------------------------------------
# EGC-S layer
# ------------------------------------------------------------------------------------------------
class EGCMessagePassingLayer(AbstractMessagePassingLayer):
    """EGC-S layer; constructor, parameters and semantics of egcmessagepassing.py:8-99:
        w      = X Wc^T + bc                                      [N, K*B]
        msg_e  = W_{t(e)} Dropout(x[src_e])                       [E, K*B*Dh]   (bias-free per-type bases)
        out[v] = sum_b w[v, k, b] * (reduce_{e -> v} msg_e)[k, b, :]   per head k, Dh = D / K
    Edge features are accepted and ignored, as in the reference.

    Inference (fp32, no gradient, torch_scatter reduce set): the bases run as the per-node table X [W_0; ...]^T or, with
    many sparse edge types, as the grouped per-edge GEMM (`_prefer_edge_path`), and ONE launch aggregates and combines
    (ops.gather_combine): the [N, K*B*Dh] aggregate never reaches memory.  Training: the same GEMMs as autograd nodes
    (per-edge input dropout folded into the edge form), the HIP segment reduce, and the combine as `dense.basis_combine`
    with its one-pass HIP backward."""

    def __init__(self, input_state_dimension: int, output_state_dimension: int, num_edge_types: int,
                 message_aggregation_function: str, num_bases: int = 4, num_heads: int = 8,
                 dropout_rate: float = 0.0):
        super().__init__()
        self.__input_state_dim = input_state_dimension
        assert output_state_dimension % num_heads == 0
        self.__aggregation_fn = message_aggregation_function
        self.__num_bases = num_bases
        self.__num_heads = num_heads
        self.__output_state_dim = output_state_dimension
        # construction order of the reference (Dropout, bases, coefficients): the same seed gives the same parameters
        self.__dropout = nn.Dropout(p=dropout_rate)
        self.__bases = nn.ModuleList(
            [nn.Linear(input_state_dimension, num_bases * output_state_dimension, bias=False)
             for _ in range(num_edge_types)])
        self.__weight_coeffs = nn.Linear(input_state_dimension, num_heads * num_bases)

    def forward(self, node_states: torch.Tensor, adjacency_lists: Adj, node_to_graph_idx,
                reference_node_ids: Dict[str, torch.Tensor],
                reference_node_graph_idx: Dict[str, torch.Tensor],
                edge_features: List[torch.Tensor]) -> torch.Tensor:
        assert len(adjacency_lists) == len(self.__bases)
        K, B, D = self.__num_heads, self.__num_bases, self.__output_state_dim
        if _on_host(node_states):
            return torch_route.egc_layer(node_states, adjacency_lists, edge_features, list(self.__bases),
                                         self.__weight_coeffs, self.__dropout, K, B, D, self.__aggregation_fn)
        if node_states.dtype in _AMP_DTYPES:
            return _amp_forward(self, node_states, adjacency_lists, edge_features, cast_features=False)   # (ignored)
        if node_states.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"EGCMessagePassingLayer: node states must be float32 / float16 / bfloat16 on the "
                                     f"GPU (got {node_states.dtype})")
        N, H, T = node_states.shape[0], self.__input_state_dim, len(adjacency_lists)
        Dh, M = D // K, B * D
        agg_fn = self.__aggregation_fn
        plan = ops.plan_for(adjacency_lists, N)
        wc = self.__weight_coeffs
        weights = [l.weight for l in self.__bases]
        p = self.__dropout.p if self.training else 0.0
        reduce_ok = agg_fn in ops.REDUCE_IDS
        edge_form = _prefer_edge_path(plan.num_edges, N, T, H, M)

        if reduce_ok and p == 0.0 and _no_grad_needed(node_states, *self.parameters()):
            coef = ops.linear(node_states, wc.weight, wc.bias)                                      # [N, K*B]
            if edge_form:
                msgs = ops.edge_linear(node_states, adjacency_lists, weights, False)              # [E, M]
                return ops.gather_combine(msgs, plan, K, B, Dh, agg_fn, coef, type_bits=0, col=plan.perm)
            return ops.gather_combine(ops.linear(node_states, _stack_detached(weights)), plan, K, B, Dh, agg_fn,
                                      coef)                                                        # table [N, T*M]

        coef = dense.linear(node_states, wc.weight, wc.bias)
        if reduce_ok and _edge_training_ok(H, M) and (p > 0 or edge_form):
            # training, edge form: grouped per-edge GEMM with the reference's per-edge input dropout folded in
            agg = segment_reduce(_train_edge_messages(self, node_states, plan, weights, False, p), plan, agg_fn)
        elif reduce_ok and p == 0.0:
            # training without dropout, few edge types: the message table and the differentiable HIP aggregation
            y = dense.linear(node_states, weights[0] if T == 1 else torch.cat(weights, dim=0))
            agg = gather_reduce_autograd(y, None, plan, M, agg_fn)
        else:
            # general per-edge path (odd widths, "mul"): message order = type-major, as the reference concatenates
            msgs = [dense.linear(self.__dropout(node_states.index_select(0, src)), lin.weight)
                    for (src, _), lin in zip(adjacency_lists, self.__bases)]
            agg = segment_reduce(torch.cat(msgs, dim=0), plan, agg_fn)
        return dense.basis_combine(agg, coef, K, B, Dh)

    def forward_sharded(self, node_states: torch.Tensor, shard) -> torch.Tensor:
        raise _lib.PtgnnAmdError("EGCMessagePassingLayer is not supported under dst-range sharding "
                                 "(ptgnn_amd.sharded); run it unsharded")

    @property
    def input_state_dimension(self) -> int:
        return self.__input_state_dim

    @property
    def output_state_dimension(self) -> int:
        return self.__output_state_dim


# ------------------------------------------------------------------------------------------------
# GraphNorm
# ------------------------------------------------------------------------------------------------
def _composed_graph_norm(node_states, node_to_graph_idx, num_graphs: int, gamma, alpha, bias, eps: float) -> torch.Tensor:
    """graphnorm.py:36-46 on the HIP `scatter_mean` of the facade plus torch's elementwise operators (their autograd
    included): widths beyond the fused kernels."""
    per_graph_mean = scatter_mean(node_states, node_to_graph_idx, dim=0, dim_size=num_graphs)
    shifted = node_states - alpha * per_graph_mean[node_to_graph_idx]
    sigma_2 = scatter_mean(torch.pow(shifted, 2), node_to_graph_idx, dim=0, dim_size=num_graphs) + eps
    return gamma * shifted / torch.sqrt(sigma_2[node_to_graph_idx]) + bias


class GraphNorm(AbstractMessagePassingLayer):
    """GraphNorm (arXiv:2009.03294); constructor, parameters and semantics of graphnorm.py:9-54.  Per graph g, per column:
        mu = mean_{i in g} x_i,   s_i = x_i - alpha * mu,   sig2 = mean_{i in g} s_i^2 + eps,   y_i = gamma * s_i / sqrt(sig2) + bias
    The number of graphs is `node_to_graph_idx.max() + 1`, as the reference's `scatter_mean` without `dim_size` reads it
    (one cached read-back per minibatch).

    GPU tensors: the fused HIP kernels of csrc/graph_norm.hip over the cached plan of the node -> graph map (any map, not
    only a sorted one) -- three reads of x and one write of y, with gradients the `_GraphNorm` autograd node and its
    two-read backward.  Widths beyond 1024 take the composed route.  CPU tensors: torch_route.graph_norm."""

    def __init__(self, input_state_dimension: int, eps: float = 1e-10):
        super().__init__()
        self.__input_state_dim = input_state_dimension
        self.__eps = eps

        self.gamma = nn.Parameter(torch.ones(1, input_state_dimension))
        self.alpha = nn.Parameter(torch.ones(1, input_state_dimension))
        self.bias = nn.Parameter(torch.zeros(1, input_state_dimension))

    def forward(self, node_states: torch.Tensor, adjacency_lists: Adj, node_to_graph_idx: torch.Tensor,
                reference_node_ids: Dict[str, torch.Tensor],
                reference_node_graph_idx: Dict[str, torch.Tensor],
                edge_features: List[torch.Tensor]) -> torch.Tensor:
        num_graphs = _num_samples(node_to_graph_idx)
        if _on_host(node_states):
            return torch_route.graph_norm(node_states, node_to_graph_idx, num_graphs, self.gamma, self.alpha, self.bias,
                                          self.__eps)
        if node_states.dtype in _AMP_DTYPES:   # AMP: fp32 inside, the caller's dtype outside
            return self.forward(node_states.float(), adjacency_lists, node_to_graph_idx, reference_node_ids,
                                reference_node_graph_idx, edge_features).to(node_states.dtype)
        if node_states.dtype != torch.float32:
            raise _lib.PtgnnAmdError(f"GraphNorm: node states must be float32 / float16 / bfloat16 on the GPU (got "
                                     f"{node_states.dtype})")
        if node_states.dim() != 2 or node_states.shape[1] != self.__input_state_dim:
            raise _lib.PtgnnAmdError(f"GraphNorm: node states [N, {self.__input_state_dim}] expected (got "
                                     f"{tuple(node_states.shape)})")
        if not ops.graph_norm_supported(self.__input_state_dim):
            return _composed_graph_norm(node_states, node_to_graph_idx, num_graphs, self.gamma, self.alpha, self.bias,
                                        self.__eps)
        plan = _index_plan(node_to_graph_idx, num_graphs)
        if _no_grad_needed(node_states, self.gamma, self.alpha, self.bias):
            return ops.graph_norm(node_states, self.gamma, self.alpha, self.bias, self.__eps, plan)
        return graph_norm_autograd(node_states, self.gamma, self.alpha, self.bias, self.__eps, plan)

    def forward_sharded(self, node_states: torch.Tensor, shard) -> torch.Tensor:
        raise NotImplementedError("GraphNorm is not supported under dst-range sharding (ptgnn_amd.sharded): the nodes of a "
                                  "graph may span ranks, and the per-graph statistics are not combined across ranks; "
                                  "run it unsharded")

    @property
    def input_state_dimension(self) -> int:
        return self.__input_state_dim

    @property
    def output_state_dimension(self) -> int:
        return self.__input_state_dim


# ------------------------------------------------------------------------------------------------
# MultiHeadSelfAttentionMessagePassing
# ------------------------------------------------------------------------------------------------
class MultiHeadSelfAttentionMessagePassing(AbstractMessagePassingLayer):
    """A transformer layer among the nodes of each graph; constructor, parameters (state_dict keys included) and
    semantics of selfattmessagepassing.py:9-136.  With kqv = W_h x, per head [keys dk | queries dk | values dv], the nodes
    of a graph are cut into windows of at most `max_num_nodes` consecutive rows (graph g owns the count_g rows after
    those of the graphs in front of it: only the COUNTS of `node_to_graph_idx` are read, as in the reference), and
        S[k, v] = key_k . query_v / sqrt(dk),  P = dropout(softmax_v(S)),  out_k = sum_v P[k, v] value_v
        a = LN1(dropout(W_s out) + x),  y = LN2(dropout(W_o relu(W_i a + b_i) + b_o) + a)
    (the row side is the key and the softmax runs over the queries -- the reference's order).  Line 119 adds ALL node
    states to the selected rows, so `target_reference != "all"` is defined only when the reference ids name every node
    once per row (R == N); anything else raises.  The result is then written back with `index_copy`, out of place: the
    caller's tensor is not mutated (the reference assigns into it).

    GPU tensors: dense.linear -> the fused block attention of csrc/block_attention.hip (the [n, n] scores never reach
    HBM; dropout on P is the stateless hash mask) -> W_s with the residual -> LayerNorm -> Linear + ReLU -> W_o with the
    residual -> LayerNorm, all HIP.  CPU tensors: torch_route.self_attention_message_passing.
    Under the `attention=True` matrix-input setting (ptgnn_amd/precision.py, off by default) the inference forward rounds
    the operands of the four Linears and of both attention products (csrc/block_attention16.hip) to the 16-bit type;
    the softmax, LayerNorms, residuals, every store and the whole training branch stay fp32."""

    def __init__(self, input_state_dimension: int, key_query_dimension: int, value_dimension: int,
                 output_dimension: int, intermediate_dimension: int, num_heads: int, dropout_rate: float = 0.0,
                 target_reference: str = "all", max_num_nodes: int = 250):
        super().__init__()
        self.__num_heads = num_heads
        self.__key_query_dim = key_query_dimension
        self.__value_dim = value_dimension
        self.__selfatt_head_transforms = nn.Linear(
            in_features=input_state_dimension, out_features=num_heads * (2 * key_query_dimension + value_dimension),
            bias=False)
        self.__summarization_layer = nn.Linear(in_features=num_heads * value_dimension, out_features=output_dimension,
                                               bias=False)
        self.__intermediate_layer = nn.Linear(in_features=output_dimension, out_features=intermediate_dimension)
        self.__output_layer = nn.Linear(in_features=intermediate_dimension, out_features=output_dimension)
        self.__layer_norm1 = nn.LayerNorm(output_dimension)
        self.__layer_norm2 = nn.LayerNorm(output_dimension)
        self.__dropout_layer = nn.Dropout(p=dropout_rate)
        self.__target_reference = target_reference
        self.__max_num_nodes = max_num_nodes

    def forward(self, node_states: torch.Tensor, adjacency_lists: Adj, node_to_graph_idx: torch.Tensor,
                reference_node_ids: Dict[str, torch.Tensor],
                reference_node_graph_idx: Dict[str, torch.Tensor],
                edge_features: List[torch.Tensor]) -> torch.Tensor:
        if self.__target_reference == "all":
            return self.__transform(node_states, node_states, node_to_graph_idx)
        ids = reference_node_ids[self.__target_reference]
        if ids.shape[0] != node_states.shape[0]:
            raise _lib.PtgnnAmdError(
                f"MultiHeadSelfAttentionMessagePassing: target_reference {self.__target_reference!r} selects "
                f"{ids.shape[0]} of {node_states.shape[0]} nodes, but selfattmessagepassing.py line 119 adds all node "
                "states to the selected rows: the layer is only defined when the reference ids cover every node")
        out = self.__transform(node_states[ids], node_states, reference_node_graph_idx[self.__target_reference])
        return node_states.index_copy(0, ids, out)

    def __transform(self, x: torch.Tensor, residual: torch.Tensor, graph_idx: torch.Tensor) -> torch.Tensor:
        heads, dk, dv = self.__num_heads, self.__key_query_dim, self.__value_dim
        w_h, w_s = self.__selfatt_head_transforms, self.__summarization_layer
        w_i, w_o, ln1, ln2 = self.__intermediate_layer, self.__output_layer, self.__layer_norm1, self.__layer_norm2
        if _on_host(x):
            # the attention=True matrix-input setting as the CPU route applies it: fp32 states, inference only (as on
            # the GPU: nothing needs a gradient, dropout inactive)
            host_dt = torch.float32
            if x.dtype == torch.float32 and not (self.training and self.__dropout_layer.p > 0) \
                    and _no_grad_needed(x, residual, *self.parameters()):
                host_dt = precision.attention_inputs(x)
            return torch_route.self_attention_message_passing(x, residual, graph_idx, w_h, w_s, w_i, w_o, ln1, ln2,
                                                              self.__dropout_layer, heads, dk, dv, self.__max_num_nodes,
                                                              inputs=host_dt)
        if x.dtype in _AMP_DTYPES:   # AMP: fp32 inside, the caller's dtype outside
            return self.__transform(x.float(), residual.float(), graph_idx).to(x.dtype)
        if x.dtype != torch.float32:
            raise _lib.PtgnnAmdError("MultiHeadSelfAttentionMessagePassing: node states must be float32 / float16 / "
                                     f"bfloat16 on the GPU (got {x.dtype})")
        if x.dim() != 2 or x.shape[1] != w_h.in_features:
            raise _lib.PtgnnAmdError(f"MultiHeadSelfAttentionMessagePassing: node states [N, {w_h.in_features}] expected "
                                     f"(got {tuple(x.shape)})")
        if not ops.block_attention_supported(dk, dv):
            raise _lib.PtgnnAmdError(f"MultiHeadSelfAttentionMessagePassing: key_query_dimension {dk} / value_dimension "
                                     f"{dv} outside the fused attention's 1..128 (there is no other GPU route)")
        if w_o.out_features > 512:
            raise _lib.PtgnnAmdError(f"MultiHeadSelfAttentionMessagePassing: output_dimension {w_o.out_features} exceeds "
                                     "the 512 columns of the LayerNorm kernel (row_epilogue)")
        if w_o.out_features != residual.shape[1]:
            raise _lib.PtgnnAmdError(f"MultiHeadSelfAttentionMessagePassing: output_dimension {w_o.out_features} must "
                                     f"equal the state dimension {residual.shape[1]} (the residual of line 119)")
        training, p = self.training, float(self.__dropout_layer.p)
        drop = p if training else 0.0
        plan = _index_plan(graph_idx, _num_samples(graph_idx))
        windows = ops.attention_windows(plan, self.__max_num_nodes)
        seed = _dropout_seed() if drop > 0 else 0
        params = [w_h.weight, w_s.weight, w_i.weight, w_i.bias, w_o.weight, w_o.bias, ln1.weight, ln1.bias, ln2.weight,
                  ln2.bias]
        if _no_grad_needed(x, residual, *params) and drop == 0:
            # float32 unless the setting was made with attention=True (ptgnn_amd/precision.py): then the four Linears and
            # both products of the attention take 16-bit operands, as under autocast in the reference
            dt = precision.attention_inputs(x)

            def w16(name: str, lin: nn.Linear):
                return _half_weights(self, name, dt, ops.HALF_KIND_LINEAR, lin.in_features, lin.out_features,
                                     lambda: lin.weight.detach().to(dt).contiguous())
            kqv = ops.linear(x, w_h.weight, inputs=dt, rounded=w16("att_w_h16", w_h))
            values, _ = ops.block_attention(kqv, windows, self.__max_num_nodes, heads, dk, dv, inputs=dt)
            a = ops.row_epilogue(ops.linear_add(values, w_s.weight, residual, inputs=dt, rounded=w16("att_w_s16", w_s)),
                                 ops.EPI_LAYERNORM, ln1.weight, ln1.bias, ln1.eps)
            hidden = ops.linear(a, w_i.weight, w_i.bias, act="relu", inputs=dt, rounded=w16("att_w_i16", w_i))
            return ops.row_epilogue(ops.linear_add(hidden, w_o.weight, a, bias=w_o.bias, inputs=dt,
                                                   rounded=w16("att_w_o16", w_o)),
                                    ops.EPI_LAYERNORM, ln2.weight, ln2.bias, ln2.eps)
        kqv = dense.linear(x, w_h.weight)
        values = block_attention_autograd(kqv, windows, self.__max_num_nodes, heads, dk, dv, drop, seed)
        a = dense.row_epilogue(self.__linear_dropout(values, w_s, None, drop) + residual, False, ln1)
        hidden = self.__linear_dropout(a, w_i, "relu", 0.0)
        return dense.row_epilogue(self.__linear_dropout(hidden, w_o, None, drop) + a, False, ln2)

    @staticmethod
    def __linear_dropout(x: torch.Tensor, lin: nn.Linear, act: Optional[str], p: float) -> torch.Tensor:
        """dropout(act(Linear(x))) as one autograd node where the widths allow, else composed from the HIP Linear."""
        y = dense.linear_act_dropout(x, lin.weight, lin.bias, act, p, p > 0)
        if y is None:
            y = dense.linear(x, lin.weight, lin.bias)
            y = torch.relu(y) if act == "relu" else y
            y = nn.functional.dropout(y, p, True) if p > 0 else y
        return y

    def forward_sharded(self, node_states: torch.Tensor, shard) -> torch.Tensor:
        raise NotImplementedError("MultiHeadSelfAttentionMessagePassing is not supported under dst-range sharding "
                                  "(ptgnn_amd.sharded): the nodes of a graph may span ranks, and attention among them is "
                                  "not combined across ranks; run it unsharded")

    @property
    def input_state_dimension(self) -> int:
        return self.__selfatt_head_transforms.in_features

    @property
    def output_state_dimension(self) -> int:
        return self.__output_layer.out_features


# ------------------------------------------------------------------------------------------------
# PNA aggregation module
# ------------------------------------------------------------------------------------------------
class PnaMessageAggregation(AbstractMessageAggregation):
    """Principal Neighbourhood Aggregation; constructor and semantics of pna_aggregation.py:13-59 (no parameters, no
    buffers).  forward(messages [E, M], message_targets [E] int64, num_nodes) -> [N, 15M]:
        A = [sum, mean, max, min, std] per target (fp32, cast to the message dtype),  out = [A | A*s | A*s']
    with s = log(in-degree + 1) / delta, s' = 1 / (s + 1e-3).

    GPU tensors: one fused HIP launch over a plan of the targets (ops.pna_aggregate; with gradients the `_PnaAggregate`
    autograd node and its one-pass HIP backward).  CPU tensors: torch_route.pna_aggregate.  Inside an
    `MlpMessagePassingLayer` the aggregation runs over the layer's own plan instead (MlpMessagePassingLayer._forward_pna),
    with GELU + LayerNorm fused into the launch for inference."""

    def __init__(self, delta: float = 1):
        super().__init__()
        self._delta = delta  # Eq. 5 of the paper

    def forward(self, messages: torch.Tensor, message_targets: torch.Tensor, num_nodes):
        if not messages.is_cuda:
            return torch_route.pna_aggregate(messages, message_targets, num_nodes, self._delta)
        if messages.dim() != 2 or message_targets.dim() != 1 or message_targets.shape[0] != messages.shape[0]:
            raise _lib.PtgnnAmdError(f"PnaMessageAggregation: messages [E, M] and 1-D targets of length E expected (got "
                                     f"{tuple(messages.shape)}, {tuple(message_targets.shape)})")
        if messages.dtype not in ops.PNA_ROUND:
            raise _lib.PtgnnAmdError(f"PnaMessageAggregation: messages must be float32 / float16 / bfloat16 on the GPU "
                                     f"(got {messages.dtype})")
        # torch_scatter semantics: a plan whose "source" column is unused; (targets, targets) gives dst = targets
        plan = ops.build_plan([(message_targets, message_targets)], int(num_nodes))
        return pna_aggregate_autograd(messages.to(torch.float32), plan, float(self._delta), round_to=messages.dtype)

    def output_state_size(self, message_input_size: int) -> int:
        return message_input_size * 5 * 3


# ------------------------------------------------------------------------------------------------
# MLP message passing layer
# ------------------------------------------------------------------------------------------------
class MlpMessagePassingLayer(AbstractMessagePassingLayer):
    """Constructor and semantics of mlpmessagepassing.py:12-125."""

    def __init__(self, input_state_dimension: int, output_state_dimension: int,
                 message_dimension: int, num_edge_types: int,
                 message_aggregation_function: Union[str, AbstractMessageAggregation],
                 message_activation: Optional[nn.Module] = nn.GELU(),
                 use_target_state_as_message_input: bool = True,
                 mlp_hidden_layers: Union[List[int], int] = 0, use_layer_norm: bool = True,
                 use_dense_layer: bool = True, dropout_rate: float = 0.0,
                 dense_activation: Optional[nn.Module] = nn.Tanh(), features_dimension: int = 0):
        super().__init__()
        self.__input_state_dim = input_state_dimension
        self.__use_target_state_as_message_input = use_target_state_as_message_input
        self.__output_state_dim = output_state_dimension
        msg_in = (2 if use_target_state_as_message_input else 1) * input_state_dimension
        self.__edge_message_transformation_layers = nn.ModuleList(
            [MLP(input_dimension=msg_in + features_dimension, output_dimension=message_dimension,
                 hidden_layers=mlp_hidden_layers) for _ in range(num_edge_types)])
        self.__aggregation_fn = message_aggregation_function
        if isinstance(message_aggregation_function, str):
            agg_size = message_dimension
        else:
            agg_size = message_aggregation_function.output_state_size(message_dimension)
        self.__message_activation = message_activation
        upd: List[nn.Module] = []
        ln = dense = act = None
        if use_layer_norm:
            ln = nn.LayerNorm(agg_size)
            upd.append(ln)
        if use_dense_layer:
            dense = nn.Linear(agg_size, output_state_dimension)
            nn.init.xavier_uniform_(dense.weight)
            upd.append(dense)
            if dense_activation is not None:
                act = dense_activation
                upd.append(act)
        drop = nn.Dropout(p=dropout_rate)
        upd.append(drop)
        # registered ONCE, under the reference's name => identical state_dict keys; the aliases below
        # bypass nn.Module registration on purpose
        self.__state_update = nn.Sequential(*upd)
        for name, mod in (("_ln", ln), ("_dense", dense), ("_dense_act", act), ("_dropout", drop)):
            object.__setattr__(self, name, mod)
        self._message_dimension = message_dimension
        self._features_dimension = features_dimension

    # -- fused path -------------------------------------------------------------------------
    def _first_weights(self) -> List[torch.Tensor]:
        return [m.linears[0].weight for m in self.__edge_message_transformation_layers]

    def _stacked_edge_weights(self, detach: bool = True, split: bool = False):
        """[(1|2)*T*M, H]: source halves of every type, then (with target state) the target halves; rebuilt
        per call (see `_stack_detached`).  `detach=False`: with gradient, for the training routes; `split`: the
        (source, target or None) stacks as two tensors."""
        ws = [w.detach() for w in self._first_weights()] if detach else self._first_weights()
        H = self.__input_state_dim
        src = [w[:, :H] for w in ws]
        dst = [w[:, H:2 * H] for w in ws] if self.__use_target_state_as_message_input else []
        if split:
            return torch.cat(src, dim=0), (torch.cat(dst, dim=0) if dst else None)
        return torch.cat(src + dst, dim=0).contiguous()

    def _table_halves(self, y: torch.Tensor, num_types: int):
        """(source term, destination term or None) of the table y = X [W^s_0; ...; W^d_0; ...]^T."""
        TM = num_types * self._message_dimension
        return y[:, :TM], (y[:, TM:] if self.__use_target_state_as_message_input else None)

    def _table_ok(self, node_states, edge_features) -> bool:
        if not isinstance(self.__aggregation_fn, str) or self.__aggregation_fn not in ops.REDUCE_IDS:
            return False                                     # aggregation modules; "mul": the seam's own kernel
        if _has_edge_features(self._features_dimension, edge_features):
            return False
        if not all(m.is_single_linear for m in self.__edge_message_transformation_layers):
            return False
        return node_states.dtype == torch.float32

    def _fused_ok(self, node_states, edge_features) -> bool:
        if not self._table_ok(node_states, edge_features):
            return False
        return (not torch.is_grad_enabled()) or _no_grad_needed(node_states, *self.parameters())

    def _epilogue(self, width: int, cap: int, cap_without_ln: bool = True) -> dict:
        """The `epilogue / ln_weight / ln_bias / ln_eps` keywords that fold the message activation and the LayerNorm
        into a launch over rows of `width`, or {} where they cannot be folded: only the stock ones are (erf GELU, affine
        LayerNorm with a bias), and only up to `cap` columns (`cap_without_ln=False`: the cap is the LayerNorm's)."""
        act, ln = self.__message_activation, self._ln
        gelu_ok = act is None or (isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none")
        ln_ok = ln is None or (ln.elementwise_affine and ln.bias is not None)
        if not (gelu_ok and ln_ok) or (width > cap and (cap_without_ln or ln is not None)):
            return {}
        return dict(epilogue=(ops.EPI_GELU if act is not None else 0) | (ops.EPI_LAYERNORM if ln is not None else 0),
                    ln_weight=ln.weight if ln is not None else None, ln_bias=ln.bias if ln is not None else None,
                    ln_eps=ln.eps if ln is not None else 1e-5)

    def _aggregate_and_update(self, ysrc, ydst, plan, col=None, type_bits=None, two_block=None) -> torch.Tensor:
        """Fused gather/reduce with GELU + LayerNorm folded into the kernel epilogue when the
        layer's activation/normalisation are the stock ones, then the dense update.  `two_block` =
        (shard, work, table_of): the sharded two-block aggregation instead (epilogue in its combine pass)."""
        M = self._message_dimension
        epi = self._epilogue(M, 512, cap_without_ln=False)
        if two_block is not None:
            from ptgnn_amd import sharded
            shard, work, table_of = two_block
            agg = sharded.aggregate_two_blocks(shard, work, table_of, M, self.__aggregation_fn, ydst=ydst, **epi)
        elif (epi and ydst is None and self._dense is not None
              and (self._dense_act is None or _kernel_act(self._dense_act) is not None)
              and not (self.training and getattr(self._dropout, "p", 0.0) > 0)
              and _no_grad_needed(ysrc, *self._dense.parameters())
              and ops.gather_update_supported(M, self._dense.out_features, plan)):
            # hidden 64 (the README's default architecture, BASELINE config 4), edge form: aggregation, GELU, LayerNorm,
            # Linear and Tanh in ONE launch -- the [N, M] aggregate never exists in memory (gather_reduce.hip)
            # (the fused launch stores 16-byte vectors: a hint whose rows are not 16-byte aligned -- the right half of a
            # concat buffer whose left half is not a multiple of 4 wide -- is declined, the residual then concatenates)
            hint = _take_output_hint(plan.num_nodes, self._dense.out_features, ysrc, vector_stores=True)
            out = ops.gather_update(ysrc, plan, self.__aggregation_fn, plan.col if col is None else col,
                                    plan.type_bits if type_bits is None else type_bits, epi["epilogue"],
                                    epi["ln_weight"], epi["ln_bias"], epi["ln_eps"],
                                    self._dense.weight, self._dense.bias, _kernel_act(self._dense_act), out=hint)
            return self._dropout(out)
        else:
            agg = ops.gather_reduce(ysrc, plan, M, self.__aggregation_fn, ydst=ydst, col=col, type_bits=type_bits, **epi)
        return self._update(agg, bool(epi))

    def _aggregate_edge_messages(self, messages, plan, inference: bool) -> torch.Tensor:
        """Aggregation + update over [E, M] messages in type-major order: the fused launches in inference (reduce set of
        the kernels, 16-byte rows), else the HIP segment-reduce seam with its autograd rule."""
        if inference and self.__aggregation_fn in ops.REDUCE_IDS and messages.shape[1] % 4 == 0:
            return self._aggregate_and_update(messages, None, plan, col=plan.perm, type_bits=0)
        return self._update(segment_reduce(messages, plan, self.__aggregation_fn), False)

    def forward_sharded(self, node_states: torch.Tensor, shard) -> torch.Tensor:
        """One layer over a dst-range shard (ptgnn_amd/sharded.py).  Table form: the source term rides the halo
        all-to-all, the destination term W_t^d x_v is purely local.  Edge form (many sparse edge types): the
        grouped per-edge GEMM reads source AND destination rows from the local table [own | halo]
        (destinations are always own rows)."""
        _check_device(node_states)
        feats = [None] * len(shard.local_adj)
        assert len(shard.local_adj) == len(self.__edge_message_transformation_layers)
        T, M, H = len(shard.local_adj), self._message_dimension, self.__input_state_dim
        if not self._table_ok(node_states, feats):
            raise _lib.PtgnnAmdError("forward_sharded needs a string aggregation and single-Linear edge "
                                     "transforms without edge features")
        use_dst = self.__use_target_state_as_message_input
        ws = self._first_weights()
        edge_form = _prefer_edge_path(*shard.form_sizes(T * M > H), T, H, M)   # one decision for the whole group
        if not self._fused_ok(node_states, feats):
            if edge_form and _edge_training_ok(H, M):
                msgs = _train_edge_messages(self, shard.exchange_autograd(node_states), shard.plan, ws, use_dst)
                return self._aggregate_edge_messages(msgs, shard.plan, False)
            w_src, w_dst = self._stacked_edge_weights(detach=False, split=True)
            ysrc = _shard_source_table_autograd(shard, node_states, w_src)
            ydst = dense.linear(node_states, w_dst) if use_dst else None
            return self._update(gather_reduce_autograd(ysrc, ydst, shard.plan, M, self.__aggregation_fn), False)

        def edge_messages(table, adj, plan):
            return ops.edge_linear(table, adj, ws, use_dst), plan.perm
        if shard.overlap and self.__aggregation_fn in _overlap_reduces():
            w = self._stacked_edge_weights()
            two_block = _shard_two_blocks(shard, node_states, w[: T * M], edge_messages if edge_form else None)
            ydst = ops.linear(node_states, w[T * M:]) if use_dst and not edge_form else None
            return self._aggregate_and_update(None, ydst, None, two_block=(shard,) + two_block)
        if edge_form:
            msgs, col = edge_messages(shard.exchange(node_states), shard.local_adj, shard.plan)
            return self._aggregate_and_update(msgs, None, shard.plan, col=col, type_bits=0)
        w = self._stacked_edge_weights()
        ysrc = _shard_source_table(shard, node_states, w[: T * M])
        ydst = ops.linear(node_states, w[T * M:]) if use_dst else None
        return self._aggregate_and_update(ysrc, ydst, shard.plan)

    def _forward_pna(self, node_states: torch.Tensor, adjacency_lists: Adj, edge_features) -> Optional[torch.Tensor]:
        """The layer with exactly `PnaMessageAggregation` (not a subclass) over its own plan; None where this route does
        not apply (edge features, deeper or biased edge MLPs, non-fp32 states: the general per-edge path, which calls
        the aggregation module).  Inference: the message table (or the grouped per-edge GEMM), ONE launch that
        aggregates, scales and applies GELU + LayerNorm(15M) -- the [N, 15M] pre-LayerNorm tensor never exists -- and the
        dense block.  Training: the differentiable message GEMMs, `_PnaAggregate`, `_update`."""
        if (_has_edge_features(self._features_dimension, edge_features)
                or not all(m.is_single_linear for m in self.__edge_message_transformation_layers)
                or node_states.dtype != torch.float32):
            return None
        N, T, M, H = node_states.shape[0], len(adjacency_lists), self._message_dimension, self.__input_state_dim
        delta = float(self.__aggregation_fn._delta)
        use_dst = self.__use_target_state_as_message_input
        ws = self._first_weights()
        plan = ops.plan_for(adjacency_lists, N)
        edge_form = _prefer_edge_path(plan.num_edges, N, T, H, M)
        if _no_grad_needed(node_states, *self.parameters()):
            epi = self._epilogue(M, 256)
            if edge_form:
                msgs = self._edge_form_messages(node_states, adjacency_lists)
                agg = ops.pna_aggregate(msgs, plan, M, delta, type_bits=0, col=plan.perm, **epi)
            else:
                ysrc, ydst = self._table_halves(self._message_table(node_states), T)
                agg = ops.pna_aggregate(ysrc, plan, M, delta, ydst=ydst, **epi)
            return self._update(agg, bool(epi))
        if not _edge_training_ok(H, M):
            return None
        # training: the grouped per-edge GEMM as one autograd node (messages in the plan's type-major order), the fused
        # aggregation with its HIP backward, then the state update
        msgs = _train_edge_messages(self, node_states, plan, ws, use_dst)
        return self._update(pna_aggregate_autograd(msgs, plan, delta), False)

    def _update(self, agg: torch.Tensor, fused_epilogue_done: bool) -> torch.Tensor:
        x = agg
        if not fused_epilogue_done:
            act, ln = self.__message_activation, self._ln
            if ((act is not None or ln is not None) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                    and self._epilogue(x.shape[1], 512)
                    and (ln is None or tuple(ln.normalized_shape) == (x.shape[-1],))):
                # training: the same GELU -> LayerNorm arithmetic as the fused inference epilogue, as one HIP
                # autograd node (forward + backward kernels of csrc/row_epilogue.hip)
                x = dense.row_epilogue(x, act is not None, ln)
            else:
                if act is not None:
                    x = act(x)
                if ln is not None:
                    x = ln(x)
        if self._dense is not None:
            act = self._dense_act
            if _no_grad_needed(x, *self._dense.parameters()):
                tanh = _kernel_act(act) == "tanh"
                hint = None
                if (tanh or act is None) and not (self.training and getattr(self._dropout, "p", 0.0) > 0):
                    # nothing follows the GEMM: it may write straight into the right half of a concat residual's result
                    hint = _take_output_hint(x.shape[0], self._dense.out_features, x)
                x = ops.linear(x, self._dense.weight, self._dense.bias, act="tanh" if tanh else None, out=hint)
                if act is not None and not tanh:
                    x = act(x)
            else:
                name = _kernel_act(act)
                if (act is None or name is not None) and isinstance(self._dropout, nn.Dropout):
                    # training: Dropout(act(Linear(x))) as one autograd node (dense._LinearActDropout)
                    fused = dense.linear_act_dropout(x, self._dense.weight, self._dense.bias, name, self._dropout.p,
                                                     self.training)
                    if fused is not None:
                        return fused
                x = dense.linear(x, self._dense.weight, self._dense.bias)
                if act is not None:
                    x = act(x)
        return self._dropout(x)

    def forward(self, node_states: torch.Tensor, adjacency_lists: Adj, node_to_graph_idx,
                reference_node_ids: Dict[str, torch.Tensor],
                reference_node_graph_idx: Dict[str, torch.Tensor],
                edge_features: List[torch.Tensor]) -> torch.Tensor:
        assert len(adjacency_lists) == len(self.__edge_message_transformation_layers), \
            "The number of adjacency lists must be equal to the number of edge types."
        if _on_host(node_states):
            return torch_route.mlp_layer(node_states, adjacency_lists, edge_features,
                                         list(self.__edge_message_transformation_layers),
                                         self.__use_target_state_as_message_input, self.__aggregation_fn,
                                         self.__message_activation, self.__state_update,
                                         inputs=self._host_matrix_inputs(node_states, edge_features))
        if node_states.dtype in _AMP_DTYPES:
            return _amp_forward(self, node_states, adjacency_lists, edge_features)

        if type(self.__aggregation_fn) is PnaMessageAggregation:
            out = self._forward_pna(node_states, adjacency_lists, edge_features)
            if out is not None:
                return out
        if self._fused_ok(node_states, edge_features):
            return self._forward_fused(node_states, adjacency_lists)
        if self._table_ok(node_states, edge_features):
            return self._forward_training(node_states, adjacency_lists)

        # deeper edge MLPs and / or edge features: the first Linear of every edge MLP as the grouped per-edge GEMM
        mlps = list(self.__edge_message_transformation_layers)
        H, hidden = self.__input_state_dim, mlps[0].linears[0].weight.shape[0]
        string_agg = isinstance(self.__aggregation_fn, str)
        if (_has_edge_features(0, edge_features) and string_agg
                and _first_linear_gemm_ok(mlps, self.training, H, differentiable=False)
                and _feat_gemm_ok(node_states, edge_features, H, hidden, *self.parameters())):
            return self._forward_features_inference(node_states, adjacency_lists, edge_features, mlps)
        has_feats = _has_edge_features(self._features_dimension, edge_features)
        gemm_ok = string_agg and _first_linear_gemm_ok(mlps, self.training, H, differentiable=True)
        if gemm_ok and has_feats and _feat_gemm_ok(node_states, edge_features, H, hidden, shapes_only=True):
            return self._forward_features_training(node_states, adjacency_lists, edge_features, mlps)
        if gemm_ok and not has_feats and node_states.dtype == torch.float32:
            return self._forward_deep_mlps(node_states, adjacency_lists, mlps)
        return self._forward_general(node_states, adjacency_lists, edge_features)

    def _forward_fused(self, node_states, adjacency_lists) -> torch.Tensor:
        """Inference, single-Linear edge transforms: grouped per-edge GEMM (many sparse edge types) or the per-node
        table, then the fused aggregation + update."""
        N, T = node_states.shape[0], len(adjacency_lists)
        plan = ops.plan_for(adjacency_lists, N)
        if _prefer_edge_path(plan.num_edges, N, T, self.__input_state_dim, self._message_dimension):
            msgs = self._edge_form_messages(node_states, adjacency_lists)
            return self._aggregate_and_update(msgs, None, plan, col=plan.perm, type_bits=0)
        ysrc, ydst = self._table_halves(self._message_table(node_states), T)
        return self._aggregate_and_update(ysrc, ydst, plan)

    def _message_table(self, node_states) -> torch.Tensor:
        """Inference, table form: [N, (1|2) T M] = X [W^s_0; ...; W^d_0; ...]^T.  Under a 16-bit matrix-input setting made
        with `mlp=True` (ptgnn_amd/precision.py) the states and the stacked weights are rounded and multiplied on the
        16-bit matrix cores, as the GGNN table form does; widths the kernel declines run fp32."""
        w = self._stacked_edge_weights()
        inputs = precision.mlp_inputs(node_states)
        w16 = _half_weights(self, "mlp_table_w16", inputs, ops.HALF_KIND_LINEAR, self.__input_state_dim, w.shape[0],
                            lambda: w.to(inputs).contiguous())
        return ops.linear(node_states, w, inputs=inputs, rounded=w16)

    def _edge_form_messages(self, node_states, adjacency_lists) -> torch.Tensor:
        """Inference, edge form: the grouped per-edge GEMM over [x[src] | x[dst]] (or x[src] alone), one row per edge in
        type-major order.  Under `mlp=True` it takes the 16-bit launch (ptgnn_amd_edge_dst_linear16, or
        ptgnn_amd_edge_linear16 without a target-state half) on a [T, M, (1|2) H] stack rounded once per forward scope;
        shapes the launch declines run fp32."""
        ws = self._first_weights()
        use_dst = self.__use_target_state_as_message_input
        H, M, T = self.__input_state_dim, self._message_dimension, len(ws)
        inputs = precision.mlp_inputs(node_states)
        w16 = None
        if inputs != torch.float32 and (ops.edge_linear16_dst_supported if use_dst
                                        else ops.edge_linear16_supported)(H, M, T, inputs):
            w16 = _scoped(self, ("mlp_edge_stack16", inputs), lambda: torch.stack([w.detach() for w in ws]).to(inputs))
        return ops.edge_linear(node_states, adjacency_lists, ws, use_dst, inputs=inputs, rounded=w16)

    def _host_matrix_inputs(self, node_states, edge_features):
        """The `mlp=True` matrix-input setting as the CPU route applies it: fp32 states, inference only (as on the GPU),
        and only for the edge transforms the GPU routes round -- single bias-free Linears without edge features."""
        if node_states.dtype != torch.float32 or _has_edge_features(self._features_dimension, edge_features):
            return torch.float32
        if not all(m.is_single_linear for m in self.__edge_message_transformation_layers):
            return torch.float32
        agg = self.__aggregation_fn
        if not (agg in ops.REDUCE_IDS if isinstance(agg, str) else type(agg) is PnaMessageAggregation):
            return torch.float32
        if torch.is_grad_enabled() and not _no_grad_needed(node_states, *self.parameters()):
            return torch.float32
        return precision.mlp_inputs(node_states)

    def _forward_training(self, node_states, adjacency_lists) -> torch.Tensor:
        """Training, single-Linear edge transforms."""
        N, T, M, H = node_states.shape[0], len(adjacency_lists), self._message_dimension, self.__input_state_dim
        plan = ops.plan_for(adjacency_lists, N)
        if _edge_training_ok(H, M) and _prefer_edge_path(plan.num_edges, N, T, H, M):
            # many sparse edge types: grouped per-edge GEMM forward + backward on HIP
            # (the edge MLPs of this layer carry no dropout: mlpmessagepassing.py:39-47)
            msgs = _train_edge_messages(self, node_states, plan, self._first_weights(),
                                        self.__use_target_state_as_message_input)
            return self._aggregate_edge_messages(msgs, plan, False)
        # dense blocks as differentiable HIP GEMM nodes, aggregation fwd + bwd on the HIP kernel
        ysrc, ydst = self._table_halves(dense.linear(node_states, self._stacked_edge_weights(detach=False)), T)
        return self._update(gather_reduce_autograd(ysrc, ydst, plan, M, self.__aggregation_fn), False)

    def _forward_features_inference(self, node_states, adjacency_lists, edge_features, mlps) -> torch.Tensor:
        """Inference with edge features: the FIRST Linear of every edge MLP as one grouped GEMM that gathers
        [x[src] | x[dst] | features] itself; the rest of the MLP (activation, further Linears) on its [E_t, .] rows."""
        plan = ops.plan_for(adjacency_lists, node_states.shape[0])
        messages = ops.edge_linear(node_states, adjacency_lists, self._first_weights(),
                                   self.__use_target_state_as_message_input, edge_feats=edge_features)
        if not all(m.is_single_linear for m in mlps):
            messages = _edge_mlp_tail(mlps, adjacency_lists, messages, differentiable=True)
        return self._aggregate_edge_messages(messages, plan, True)

    def _forward_features_training(self, node_states, adjacency_lists, edge_features, mlps) -> torch.Tensor:
        """Training with edge features: the first Linear of every edge MLP as ONE differentiable grouped GEMM that
        gathers [x[src] | x[dst] | features] itself (scatter._EdgeLinearFeat); the rest of each MLP on the type's rows."""
        plan = ops.plan_for(adjacency_lists, node_states.shape[0])
        hid = edge_linear_feat_autograd(node_states, plan, self._first_weights(),
                                        self.__use_target_state_as_message_input, edge_features)
        messages = _edge_mlp_tail(mlps, adjacency_lists, hid, differentiable=True, single_block_as_is=True)
        return self._aggregate_edge_messages(messages, plan, False)

    def _forward_deep_mlps(self, node_states, adjacency_lists, mlps) -> torch.Tensor:
        """Deeper edge MLPs (mlp_hidden_layers > 0, mlp.py:50-77) without edge features: the FIRST Linear of every edge
        type is the grouped per-edge GEMM (it gathers [x[src] | x[dst]] itself: no index_select, no [E, 2H] concat --
        inference and training alike, `_EdgeLinear` carries the gradients); the rest of each MLP runs on the type's
        [E_t, hidden] rows on the HIP Linear."""
        plan = ops.plan_for(adjacency_lists, node_states.shape[0])
        grad = not _no_grad_needed(node_states, *self.parameters())
        use_dst = self.__use_target_state_as_message_input
        if grad:
            hid = _train_edge_messages(self, node_states, plan, self._first_weights(), use_dst, key="edge_w0")
        else:
            hid = ops.edge_linear(node_states, adjacency_lists, self._first_weights(), use_dst)
        messages = _edge_mlp_tail(mlps, adjacency_lists, hid, differentiable=grad)
        return self._aggregate_edge_messages(messages, plan, not grad)

    def _forward_general(self, node_states, adjacency_lists, edge_features) -> torch.Tensor:
        """General per-edge path: torch gathers / concatenates the rows, every Linear on the HIP GEMM."""
        all_targets, all_messages = [], []
        for (src, dst), feats, edge_mlp in zip(adjacency_lists, edge_features,
                                               self.__edge_message_transformation_layers):
            all_targets.append(dst)
            inp = node_states.index_select(0, src)
            if self.__use_target_state_as_message_input:
                inp = torch.cat([inp, node_states.index_select(0, dst)], dim=-1)
            if feats is not None and feats.shape[-1] > 0:
                inp = torch.cat([inp, feats.to(inp.dtype)], dim=-1)
            all_messages.append(_run_mlp(edge_mlp, inp))                           # HIP GEMMs
        messages = torch.cat(all_messages, dim=0)
        if isinstance(self.__aggregation_fn, str):
            plan = ops.plan_for(adjacency_lists, node_states.shape[0])
            return self._aggregate_edge_messages(messages, plan, False)
        agg = self.__aggregation_fn(messages=messages, message_targets=torch.cat(all_targets, dim=0),
                                    num_nodes=node_states.shape[0])
        return self._update(agg, False)

    @property
    def input_state_dimension(self) -> int:
        return self.__input_state_dim

    @property
    def output_state_dimension(self) -> int:
        return self.__output_state_dim

    def export_weights(self) -> Dict:
        c = lambda t: None if t is None else t.detach().cpu()  # noqa: E731
        return {"kind": "mlp",
                "edge_mlp": [[l.weight.detach().cpu() for l in m.linears]
                             for m in self.__edge_message_transformation_layers],
                "use_target": self.__use_target_state_as_message_input, "agg": self.__aggregation_fn,
                "gelu": self.__message_activation is not None,
                "ln_w": c(self._ln.weight) if self._ln is not None else None,
                "ln_b": c(self._ln.bias) if self._ln is not None else None,
                "dense_w": c(self._dense.weight) if self._dense is not None else None,
                "dense_b": c(self._dense.bias) if self._dense is not None else None,
                "tanh": self._dense_act is not None}


# ------------------------------------------------------------------------------------------------
# residual layers (residuallayers.py): elementwise glue that every shipped stack uses
# ------------------------------------------------------------------------------------------------
class _ResidualOriginLayer(AbstractMessagePassingLayer):
    def __init__(self, input_dim: int, target_layer):
        super().__init__()
        self.__target_layer = target_layer   # registered like the reference (same state_dict keys)
        self.__input_dim = input_dim

    def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                reference_node_graph_idx, edge_features):
        self.__target_layer._original_input = node_states
        return node_states

    @property
    def input_state_dimension(self) -> int:
        return self.__input_dim

    @property
    def output_state_dimension(self) -> int:
        return self.__input_dim


class _ResidualBase(AbstractMessagePassingLayer):
    def __init__(self, input_dim: int):
        super().__init__()
        self._original_input = None
        self._input_dim = input_dim

    def pass_through_dummy_layer(self) -> _ResidualOriginLayer:
        return _ResidualOriginLayer(self._input_dim, target_layer=self)

    def _pop(self) -> torch.Tensor:
        assert self._original_input is not None, "Initial Pass Through Layer was not used."
        x, self._original_input = self._original_input, None
        return x

    @property
    def input_state_dimension(self) -> int:
        return self._input_dim


class MeanResidualLayer(_ResidualBase):
    def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                reference_node_graph_idx, edge_features):
        return (self._pop() + node_states) * 0.5   # == stack(..).mean(-1) bit for bit (/2 is exact)

    @property
    def output_state_dimension(self) -> int:
        return self._input_dim


class ConcatResidualLayer(_ResidualBase):
    def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                reference_node_graph_idx, edge_features):
        orig = self._pop()
        buf = getattr(node_states, "_ptgnn_amd_concat_buffer", None)
        if (buf is not None and buf.shape[1] == orig.shape[1] + node_states.shape[1] and buf.dtype == orig.dtype
                and node_states.data_ptr() == buf[:, orig.shape[1]:].data_ptr()):
            # the previous layer wrote straight into the right half of the result (see set_output_hint)
            buf[:, : orig.shape[1]].copy_(orig)
            return buf
        return torch.cat((orig, node_states), dim=-1)

    def make_result_buffer(self, num_nodes: int, next_dim: int, like: torch.Tensor) -> torch.Tensor:
        return torch.empty(num_nodes, self._input_dim + next_dim, dtype=like.dtype, device=like.device)

    @property
    def output_state_dimension(self) -> int:
        return 2 * self._input_dim


class LinearResidualLayer(_ResidualBase):
    def __init__(self, state_dimension1: int, state_dimension2: int, target_state_size: int,
                 dropout_rate: float = 0.0):
        super().__init__(state_dimension1)
        self.__input_dim2 = state_dimension2
        self.__linear_combination = nn.Linear(state_dimension1 + state_dimension2, target_state_size,
                                              bias=False)
        self.__dropout = nn.Dropout(p=dropout_rate)

    def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                reference_node_graph_idx, edge_features):
        x = torch.cat((self._pop(), node_states), dim=-1)
        lin = self.__linear_combination
        if _on_host(x):
            return self.__dropout(lin(x))
        if x.dtype in _AMP_DTYPES:
            return self.__dropout(dense.linear(x.float(), lin.weight).to(x.dtype))
        if _no_grad_needed(x, lin.weight):
            return self.__dropout(ops.linear(x, lin.weight))
        return self.__dropout(dense.linear(x, lin.weight))

    @property
    def input_state_dimension(self) -> int:
        return self.__input_dim2

    @property
    def output_state_dimension(self) -> int:
        return self.__linear_combination.out_features
