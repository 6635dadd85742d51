"""The HOST-TENSOR route of the drop-in layers and of the `torch_scatter` facade: plain torch operators, for tensors
that live on the CPU.

Why it exists.  The reference's own inference entry restores a model and runs it on "cpu"
(ptgnn/implementations/typilus/predict.py:25-27), and its trainer runs on the CPU when no GPU is visible
(ptgnn/baseneuralmodel/trainer.py:392-395).  A checkpoint whose layers are `ptgnn_amd` classes has to survive
both, so the layers dispatch on the DEVICE OF THEIR INPUT exactly like a torch operator does:

    * tensors on the GPU  -> libptgnn_amd.so (HIP kernels).  ALWAYS.  A missing / stale library or an entry
      point that fails raises `PtgnnAmdError`; nothing on that side ever reaches this file (every function here
      starts with `_host_only`, which raises for a device tensor), so a GPU run can not silently become a torch run.
    * tensors on the CPU  -> this file.

This is product code (it ships in `ptgnn_amd/`), written against the reference's semantics
(gatedmessagepassing.py:37-69, mlpmessagepassing.py:68-117, abstractmessagepassing.py:38-50,
globalgraphexchange.py:29-45, residuallayers.py) and torch_scatter 2.0.x's published behaviour; it imports nothing
from `oracle/` (the test-side restatement), and `tests/dropin_check.py` compares it with the reference's own
layers on the reference's own container and batcher.
"""
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from ptgnn_amd import _lib


def _host_only(*tensors) -> None:
    for t in tensors:
        if t is not None and t.is_cuda:
            raise _lib.PtgnnAmdError("ptgnn_amd.torch_route is the CPU-tensor route; a GPU tensor must take the HIP "
                                     "kernels (this is a bug in the caller, not a fallback)")


# ------------------------------------------------------------------------------------------------------------------
# segment reduce with torch_scatter's semantics over rows [E, D] and a 1-D int64 index
# ------------------------------------------------------------------------------------------------------------------
class _SegmentProduct(torch.autograd.Function):
    """reduce="mul": product per segment in element order, empty segments 1; backward as torch_scatter's
    ScatterMul: (grad_out * out)[index] / src with 0 / 0 -> 0."""

    @staticmethod
    def forward(ctx, rows, index, n):
        out = torch.ones(n, rows.shape[1], dtype=rows.dtype).scatter_reduce_(
            0, index.unsqueeze(1).expand_as(rows), rows, "prod", include_self=True)
        ctx.save_for_backward(rows, index, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rows, index, out = ctx.saved_tensors
        g = (grad_out * out).index_select(0, index) / rows
        return g.masked_fill(g.isnan(), 0.0), None, None


def _winner_positions(rows: torch.Tensor, index: torch.Tensor, best: torch.Tensor, n: int) -> torch.Tensor:
    """torch_scatter's arg_out: the FIRST element (in element order) that attains the segment's extremum, per column;
    `E` for a segment without elements."""
    E, D = rows.shape
    pos = torch.arange(E, dtype=torch.int64).unsqueeze(1).expand(E, D)
    b = best.index_select(0, index)
    attained = rows == b
    if rows.is_floating_point():     # a NaN in a segment IS its extremum (torch_scatter and the reference propagate it)
        attained = attained | (rows.isnan() & b.isnan())
    cand = torch.where(attained, pos, torch.full_like(pos, E))
    arg = torch.full((n, D), E, dtype=torch.int64)
    return arg.scatter_reduce_(0, index.unsqueeze(1).expand(E, D), cand, reduce="amin", include_self=True)


def segment(rows: torch.Tensor, index: torch.Tensor, n: int, reduce: str, return_arg: bool = False):
    """out[s] = reduce over {rows[e] : index[e] == s}, [n, D]; sums fold in element order (the order the reference's
    CPU scatter_add_ folds them in).  Differentiable with torch_scatter's rules: max / min route the gradient to the
    single recorded winner (not spread over ties like torch's own amax)."""
    _host_only(rows, index)
    E, D = rows.shape
    if reduce in ("sum", "add"):
        out = torch.zeros(n, D, dtype=rows.dtype).index_add_(0, index, rows)
    elif reduce == "mean":
        total = torch.zeros(n, D, dtype=rows.dtype).index_add_(0, index, rows)
        count = torch.bincount(index, minlength=n)[:n].clamp_(min=1)
        out = total / count.to(rows.dtype).unsqueeze(1) if rows.is_floating_point() else \
            total.div(count.unsqueeze(1), rounding_mode="floor")
    elif reduce in ("max", "min"):
        with torch.no_grad():
            best = torch.zeros(n, D, dtype=rows.dtype).scatter_reduce_(
                0, index.unsqueeze(1).expand(E, D), rows.detach(), "amax" if reduce == "max" else "amin",
                include_self=False)
            arg = _winner_positions(rows.detach(), index, best, n)
        if E == 0:
            out = torch.zeros(n, D, dtype=rows.dtype) + rows.sum() * 0
        else:
            picked = rows.gather(0, arg.clamp(max=E - 1))            # gradient reaches the winner only
            out = torch.where(arg < E, picked, torch.zeros((), dtype=rows.dtype))
        if return_arg:
            return out, arg
    elif reduce == "mul":
        out = _SegmentProduct.apply(rows, index, n)
    else:
        raise ValueError(f"unknown aggregation function {reduce!r}")
    if return_arg:
        raise ValueError("arg is defined for max / min only")
    return out


def graph_norm(node_states: torch.Tensor, node_to_graph_idx: torch.Tensor, num_graphs: int, gamma: torch.Tensor,
               alpha: torch.Tensor, bias: torch.Tensor, eps: float) -> torch.Tensor:
    """graphnorm.py:36-46, the reference's operator sequence (scatter_mean = `segment(..., "mean")`)."""
    _host_only(node_states, node_to_graph_idx)
    per_graph_mean = segment(node_states, node_to_graph_idx, num_graphs, "mean")          # [num_graphs, D]
    shifted = node_states - alpha * per_graph_mean[node_to_graph_idx]                     # [num_nodes, D]
    sigma_2 = segment(torch.pow(shifted, 2), node_to_graph_idx, num_graphs, "mean") + eps  # [num_graphs, D]
    return gamma * shifted / torch.sqrt(sigma_2[node_to_graph_idx]) + bias


def attention_window_bounds(node_to_graph_idx: torch.Tensor, max_num_nodes: int):
    """[(first row, end row)] of the windows of selfattmessagepassing.py:59-75: graph g owns the count_g rows after those
    of the graphs in front of it (only the counts of the map are read) and is cut every max_num_nodes rows."""
    counts = torch.bincount(node_to_graph_idx).tolist() if node_to_graph_idx.numel() else []
    bounds, first = [], 0
    for count in counts:
        bounds += [(first + lo, first + min(lo + max_num_nodes, count)) for lo in range(0, count, max_num_nodes)]
        first += count
    return bounds


def block_attention(kqv: torch.Tensor, bounds, num_heads: int, dk: int, dv: int, dropout_p: float = 0.0,
                    training: bool = False, inputs: torch.dtype = torch.float32) -> torch.Tensor:
    """selfattmessagepassing.py:104-117 in the dtype of `kqv` [N, heads (2 dk + dv)]: per window and head
    softmax_v(key_k . query_v / sqrt(dk)), dropout, times the values -> [N, heads dv].
    `inputs` = torch.bfloat16 / torch.float16: k, q, v and the probabilities in front of the value product are rounded
    to that type with torch (the softmax itself stays fp32)."""
    n = kqv.shape[0]
    if inputs != torch.float32:
        kqv = _rounded(kqv, inputs)
    per_head = kqv.reshape(n, num_heads, 2 * dk + dv).permute(1, 0, 2)             # [heads, N, 2 dk + dv]
    pieces = []
    for lo, hi in bounds:
        block = per_head[:, lo:hi]
        keys, queries, values = block[..., :dk], block[..., dk:2 * dk], block[..., 2 * dk:]
        probs = torch.softmax(keys @ queries.transpose(1, 2) / dk ** 0.5, dim=-1)   # [heads, key, query]
        probs = nn.functional.dropout(probs, dropout_p, training)
        if inputs != torch.float32:
            probs = _rounded(probs, inputs)
        pieces.append(probs @ values)                                               # [heads, n, dv]
    if not pieces:
        return kqv.new_zeros(n, num_heads * dv)
    return torch.cat(pieces, dim=1).permute(1, 0, 2).reshape(n, num_heads * dv)


def self_attention_message_passing(node_states: torch.Tensor, residual_states: torch.Tensor,
                                   node_to_graph_idx: torch.Tensor, head_transforms: nn.Linear, summarization: nn.Linear,
                                   intermediate: nn.Linear, output: nn.Linear, layer_norm1: nn.LayerNorm,
                                   layer_norm2: nn.LayerNorm, dropout: nn.Module, num_heads: int, dk: int, dv: int,
                                   max_num_nodes: int, inputs: torch.dtype = torch.float32) -> torch.Tensor:
    """MultiHeadSelfAttentionMessagePassing.forward (selfattmessagepassing.py:92-123) on torch's operators, any dtype:
    `node_states` are the rows that attend (line 89), `residual_states` what line 119 adds.
    `inputs` = torch.bfloat16 / torch.float16 (the caller's `attention=True` matrix-input setting; fp32 states,
    inference only): the operands the GPU route rounds are rounded here with torch and multiplied by the fp32 operators
    -- the inputs and weights of the four Linears, k, q and v, and the probabilities in front of the value product.  This
    route rounds the NORMALISED probabilities, as autocast does; the kernel (csrc/block_attention16.hip) rounds the
    unnormalised ones and divides by the unrounded sum.  Either way every probability is within one unit roundoff of
    the 16-bit type (2^-8 / 2^-11 relative) of its unrounded value.  Softmax, LayerNorms, residuals, bias and ReLU stay
    fp32."""
    _host_only(node_states, node_to_graph_idx)
    if inputs == torch.float32:
        def lin(layer, x):
            return layer(x)
    else:
        def lin(layer, x):
            return nn.functional.linear(_rounded(x, inputs), _rounded(layer.weight, inputs), layer.bias)
    kqv = lin(head_transforms, node_states)
    bounds = attention_window_bounds(node_to_graph_idx, max_num_nodes)
    values = block_attention(kqv, bounds, num_heads, dk, dv, float(getattr(dropout, "p", 0.0)), dropout.training,
                             inputs=inputs)
    attention_output = layer_norm1(dropout(lin(summarization, values)) + residual_states)
    hidden = nn.functional.relu(lin(intermediate, attention_output))
    return layer_norm2(dropout(lin(output, hidden)) + attention_output)


# ------------------------------------------------------------------------------------------------------------------
# torch_scatter-shaped entry points (any `dim`, 1-D or broadcastable index) for host tensors
# ------------------------------------------------------------------------------------------------------------------
def _flatten(src: torch.Tensor, index: torch.Tensor, dim: int):
    """-> (rows [E', D'], index' [E'], restore(out_rows, n) -> tensor of src's layout with size n along dim,
    columns per segment id).  A 1-D index along `dim` keeps one segment id per slice; a wider index (torch_scatter
    broadcasts it over the trailing dimensions) gets one segment id per (index value, column)."""
    dim = dim % src.dim() if src.dim() else 0
    moved = src.movedim(dim, 0)
    tail = tuple(moved.shape[1:])
    width = 1
    for d in tail:
        width *= int(d)
    if index.dim() == 1:
        rows = moved.reshape(moved.shape[0], width)

        def restore(out_rows, n):
            return out_rows.reshape((n,) + tail).movedim(0, dim)
        return rows, index, 1, restore
    idx = index
    for _ in range(idx.dim(), src.dim()):
        idx = idx.unsqueeze(-1)
    idx = idx.expand(src.shape).movedim(dim, 0).reshape(moved.shape[0], width)    # [E, C]
    C = idx.shape[1]
    seg = (idx * C + torch.arange(C, dtype=torch.int64).unsqueeze(0)).reshape(-1)
    rows = moved.reshape(-1, 1)

    def restore(out_rows, n):
        return out_rows.reshape((n,) + tail).movedim(0, dim)
    return rows, seg, C, restore


def _size(index: torch.Tensor, dim_size) -> int:
    if dim_size is not None:
        return int(dim_size)
    return int(index.max()) + 1 if index.numel() else 0


def scatter(src, index, dim: int = -1, out=None, dim_size=None, reduce: str = "sum", return_arg: bool = False):
    _host_only(src, index)
    if out is not None:
        raise _lib.PtgnnAmdError("ptgnn_amd.scatter: the `out=` form is not supported")
    n = _size(index, dim_size)
    rows, seg, C, restore = _flatten(src, index, dim)
    res = segment(rows, seg, n * C, reduce, return_arg=return_arg)
    if not return_arg:
        return restore(res, n)
    vals, arg = res
    if C > 1:   # positions were counted over the flattened (element, column) pairs: back to the element index
        E = src.shape[dim % src.dim()]
        arg = torch.where(arg < rows.shape[0], arg // C, torch.full_like(arg, E))
    return restore(vals, n), restore(arg, n)


def _expand_index(index, src, dim):
    dim = dim % src.dim()
    idx = index
    if idx.dim() == 1:
        shape = [1] * src.dim()
        shape[dim] = idx.shape[0]
        idx = idx.view(shape)
    else:
        for _ in range(idx.dim(), src.dim()):
            idx = idx.unsqueeze(-1)
    return idx.expand(src.shape), dim


def scatter_log_softmax(src, index, dim: int = -1, eps: float = 1e-12, dim_size=None):
    idx, dim = _expand_index(index, src, dim)
    with torch.no_grad():
        shift = scatter(src.detach(), index, dim, None, dim_size, "max").gather(dim, idx)
    rec = src - shift
    total = scatter(rec.exp(), index, dim, None, dim_size, "sum")
    return rec - (total + eps).log().gather(dim, idx)


def scatter_softmax(src, index, dim: int = -1, eps: float = 1e-12, dim_size=None):
    idx, dim = _expand_index(index, src, dim)
    with torch.no_grad():
        shift = scatter(src.detach(), index, dim, None, dim_size, "max").gather(dim, idx)
    e = (src - shift).exp()
    total = scatter(e, index, dim, None, dim_size, "sum")
    return e / (total.gather(dim, idx) + eps)


def scatter_logsumexp(src, index, dim: int = -1, out=None, dim_size=None, eps: float = 1e-12):
    """torch_scatter.composite.scatter_logsumexp (2.0.x): the per-segment maximum is taken over a -inf initialised
    buffer, so a segment without elements answers log(eps) + (-inf) = -inf."""
    if out is not None:
        raise _lib.PtgnnAmdError("ptgnn_amd.scatter: the `out=` form is not supported")
    idx, dim = _expand_index(index, src, dim)
    n = _size(index, dim_size)
    with torch.no_grad():
        vals, arg = scatter(src.detach(), index, dim, None, n, "max", return_arg=True)
        E = src.shape[dim]
        top = torch.where(arg < E, vals, torch.full_like(vals, float("-inf")))
        shift = top.gather(dim, idx)
    rec = src - shift
    rec = rec.masked_fill(rec.isnan(), float("-inf"))
    total = scatter(rec.exp(), index, dim, None, n, "sum")
    return (total + eps).log() + top


def scatter_std(src, index, dim: int = -1, out=None, dim_size=None, unbiased: bool = True):
    """torch_scatter.scatter_std (2.0.x): sqrt(sum (x - mean)^2 / (max(count - 1, 1) + 1e-6))."""
    if out is not None:
        raise _lib.PtgnnAmdError("ptgnn_amd.scatter: the `out=` form is not supported")
    idx, dim = _expand_index(index, src, dim)
    n = _size(index, dim_size)
    count = scatter(torch.ones_like(src), index, dim, None, n, "sum").clamp(min=1)
    mean = scatter(src, index, dim, None, n, "sum") / count
    dev = src - mean.gather(dim, idx)
    ssq = scatter(dev * dev, index, dim, None, n, "sum")
    if unbiased:
        count = (count - 1).clamp(min=1)
    return (ssq / (count + 1e-6)).sqrt()


# ------------------------------------------------------------------------------------------------------------------
# layer bodies
# ------------------------------------------------------------------------------------------------------------------
def aggregate(messages: torch.Tensor, targets: torch.Tensor, num_nodes: int, reduce: str) -> torch.Tensor:
    """abstractmessagepassing.py:38-50: fp32 scatter whatever the message dtype (AMP), result back in that dtype."""
    return segment(messages.to(torch.float32), targets, int(num_nodes), reduce).to(messages.dtype)


def pna_aggregate(messages: torch.Tensor, targets: torch.Tensor, num_nodes: int, delta: float = 1) -> torch.Tensor:
    """pna_aggregation.py:27-56 on host tensors, in the reference's operator order: fp32 sum / mean / max / min / "std"
    of the messages per target, cast to the message dtype, then the degree scalers (the result promotes to float32
    for half / bfloat16 messages, as there)."""
    _host_only(messages, targets)
    n = int(num_nodes)
    degree = segment(torch.ones_like(targets).unsqueeze(1), targets, n, "sum").squeeze(1)
    msg_dtype = messages.dtype
    m = messages.to(torch.float32)
    sum_agg = segment(m, targets, n, "sum")
    mean_agg = sum_agg / (degree.unsqueeze(-1) + 1e-5)
    max_agg = segment(m, targets, n, "max")
    min_agg = segment(m, targets, n, "min")
    std_components = torch.relu(m.pow(2) - mean_agg[targets].pow(2)) + 1e-10
    std = torch.sqrt(segment(std_components, targets, n, "sum"))
    all_aggregations = torch.cat([sum_agg, mean_agg, max_agg, min_agg, std], dim=-1).to(msg_dtype)
    scaler_p1 = torch.log(degree.float() + 1).unsqueeze(-1) / delta
    scaler_m1 = 1 / (scaler_p1 + 1e-3)
    return torch.cat([all_aggregations, all_aggregations * scaler_p1, all_aggregations * scaler_m1], dim=-1)


def _message_inputs(node_states, adjacency_lists, edge_features, with_target: bool):
    for (src, dst), feats in zip(adjacency_lists, edge_features):
        parts = [node_states.index_select(0, src)]
        if with_target:
            parts.append(node_states.index_select(0, dst))
        if feats is not None:
            parts.append(feats)
        yield parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)


def _rounded(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """`t` rounded to a 16-bit type and back: the value the 16-bit matrix cores multiply (ptgnn_amd/precision.py)."""
    return t.to(dtype).float()


def ggnn_layer(node_states, adjacency_lists, edge_features, edge_linears: Sequence[nn.Linear], dropout: nn.Module,
               gru: nn.GRUCell, reduce: str, inputs: torch.dtype = torch.float32) -> torch.Tensor:
    """gatedmessagepassing.py:46-69 on host tensors: per type W_t . Dropout([x_src ; f_e]), type-major messages,
    segment reduce onto the targets, GRUCell(aggregate, state).
    `inputs` = torch.bfloat16 / torch.float16 (the caller's matrix-input setting, inference only): the operands the GPU
    routes round are rounded here with torch and multiplied by the fp32 operators -- the message Linear's (without edge
    features: the GPU's table form; with them the per-edge GEMM stays fp32 there and here) and the GRU gate GEMMs', with
    the unrounded state in the blend."""
    _host_only(node_states)
    if inputs == torch.float32:
        msgs = [lin(dropout(inp)) for inp, lin in
                zip(_message_inputs(node_states, adjacency_lists, edge_features, False), edge_linears)]
    else:
        plain = all(f is None or f.shape[-1] == 0 for f in edge_features)
        msgs = [nn.functional.linear(_rounded(inp, inputs), _rounded(lin.weight, inputs)) if plain else lin(inp)
                for inp, lin in zip(_message_inputs(node_states, adjacency_lists, edge_features, False), edge_linears)]
    targets = torch.cat([d for _, d in adjacency_lists])
    agg = aggregate(torch.cat(msgs, dim=0), targets, node_states.shape[0], reduce)
    if inputs == torch.float32:
        return gru(agg, node_states)
    gi = nn.functional.linear(_rounded(agg, inputs), _rounded(gru.weight_ih, inputs), gru.bias_ih)
    gh = nn.functional.linear(_rounded(node_states, inputs), _rounded(gru.weight_hh, inputs), gru.bias_hh)
    (i_r, i_z, i_n), (h_r, h_z, h_n) = gi.chunk(3, dim=1), gh.chunk(3, dim=1)
    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    return (1.0 - z) * n + z * node_states


def mlp_layer(node_states, adjacency_lists, edge_features, edge_mlps: Sequence[nn.Module], with_target: bool,
              aggregation, activation: Optional[nn.Module], state_update: nn.Module,
              inputs: torch.dtype = torch.float32) -> torch.Tensor:
    """mlpmessagepassing.py:80-117 on host tensors.
    `inputs` = torch.bfloat16 / torch.float16 (the caller's `mlp=True` matrix-input setting; inference with single
    bias-free Linear edge transforms and no edge features only): the operands the GPU routes round -- the node states and
    the message Linears' weights -- are rounded here with torch and multiplied by the fp32 operator; everything after the
    messages stays as it is."""
    _host_only(node_states)
    if inputs == torch.float32:
        msgs = [mlp(inp) for inp, mlp in
                zip(_message_inputs(node_states, adjacency_lists, edge_features, with_target), edge_mlps)]
    else:
        msgs = [nn.functional.linear(inp, _rounded(mlp.linears[0].weight, inputs)) for inp, mlp in
                zip(_message_inputs(_rounded(node_states, inputs), adjacency_lists, edge_features, with_target),
                    edge_mlps)]
    messages = torch.cat(msgs, dim=0)
    targets = torch.cat([d for _, d in adjacency_lists], dim=0)
    if isinstance(aggregation, str):
        agg = aggregate(messages, targets, node_states.shape[0], aggregation)
    else:
        agg = aggregation(messages=messages, message_targets=targets, num_nodes=node_states.shape[0])
    if activation is not None:
        agg = activation(agg)
    return state_update(agg)


def egc_layer(node_states, adjacency_lists, edge_features, bases: Sequence[nn.Linear], weight_coeffs: nn.Linear,
              dropout: nn.Module, num_heads: int, num_bases: int, output_dim: int, reduce: str) -> torch.Tensor:
    """egcmessagepassing.py:63-91 on host tensors, in the reference's operator order: node coefficients, then per type
    bases(Dropout(x_src)) as [E_t, K, B, Dh] (edge features are zipped over and ignored, as there), fp32 segment reduce
    onto the targets, (agg * w).sum over the bases."""
    _host_only(node_states)
    node_weights = weight_coeffs(node_states).reshape(-1, num_heads, num_bases, 1)
    targets, messages = [], []
    for (src, dst), _features, lin in zip(adjacency_lists, edge_features, bases):
        targets.append(dst)
        inp = dropout(nn.functional.embedding(src, node_states))
        messages.append(lin(inp).reshape(-1, num_heads, num_bases, output_dim // num_heads))
    msgs = torch.cat(messages, dim=0)
    agg = aggregate(msgs.reshape(msgs.shape[0], -1), torch.cat(targets, dim=0), node_states.shape[0], reduce)
    agg = agg.reshape(-1, num_heads, num_bases, output_dim // num_heads)
    return (agg * node_weights).sum(axis=-2).reshape(-1, output_dim)


def attention_summary(x: torch.Tensor, index: torch.Tensor, num_samples: int, queries: torch.Tensor,
                      key_weight: torch.Tensor, value_weight: Optional[torch.Tensor], output_weight: torch.Tensor,
                      num_heads: int, single_head: bool) -> torch.Tensor:
    """SelfAttentionVarSizedElementReduce.forward (varsizedsummary.py:99-113, `single_head`) and
    MultiheadSelfAttentionVarSizedElementReduce.forward (:140-178) after the query summariser, in the reference's
    operator order on host tensors."""
    _host_only(x, index, queries)
    F = nn.functional
    n = int(num_samples)
    queries_all = queries[index]                                                   # [N, hidden]
    keys = F.linear(x, key_weight)                                                 # [N, hidden]
    if single_head:
        scores = torch.einsum("vh,vh->v", queries_all, keys)
        probs = torch.exp(scatter_log_softmax(scores, index, dim=0, eps=0))
        return scatter(F.linear(x, output_weight) * probs.unsqueeze(-1), index, 0, None, n, "sum")
    N = queries_all.shape[0]
    queries_all = queries_all.reshape(N, num_heads, queries_all.shape[1] // num_heads)
    keys = keys.reshape(keys.shape[0], num_heads, keys.shape[1] // num_heads)
    scores = torch.einsum("bhk,bhk->bh", queries_all, keys) / math.sqrt(keys.shape[-1])
    probs = torch.exp(scatter_log_softmax(scores, index, dim=0, eps=0))           # [N, heads]
    if value_weight is not None:
        values = F.linear(x, value_weight)
        outputs = probs.unsqueeze(-1) * values.reshape(values.shape[0], num_heads, values.shape[1] // num_heads)
    else:
        outputs = probs.unsqueeze(-1) * x.unsqueeze(1)                             # [N, heads, D]
    per_sample = scatter(outputs.reshape(outputs.shape[0], -1), index, 0, None, n, "sum")
    return F.linear(per_sample, output_weight)


def subtoken_embed(token_idxs: torch.Tensor, lengths: torch.Tensor, table: torch.Tensor, kind: str) -> torch.Tensor:
    """The pool of SubtokenUnitEmbedder.forward (strelementrepresentationmodel.py:67-82) in the reference's operator order
    on host tensors: [B, D] from the [B, max_num_subtokens] ids and the [B] lengths."""
    _host_only(token_idxs, lengths, table)
    embedded = nn.functional.embedding(token_idxs, table)                          # [B, max_num_subtokens, D]
    mask = torch.arange(embedded.shape[1], device=lengths.device).unsqueeze(0) < lengths.unsqueeze(-1)
    if kind == "mean":
        embedded = embedded * mask.unsqueeze(-1).float()
        return embedded.sum(dim=-2) / (lengths.unsqueeze(-1).float() + 1e-10)
    if kind == "sum":
        embedded = embedded * mask.unsqueeze(-1).float()
        return embedded.sum(dim=-2)
    if kind == "max":
        embedded.masked_fill_(mask=~mask.unsqueeze(-1), value=-math.inf)
        return embedded.max(dim=-2)[0]
    raise ValueError(f'Unrecognized subtoken combination "{kind}".')


def char_cnn(chars: torch.Tensor, num_chars: int, conv1: nn.Conv1d, conv2: nn.Conv1d, conv3: nn.Conv1d) -> torch.Tensor:
    """The trunk of CharUnitEmbedder.forward (strelementrepresentationmodel.py:133-141) on host tensors, operator for
    operator: one-hot characters as the channels of a [B, C, L] float signal, three convolutions with a ReLU in front of
    the second and the third, the maximum over the remaining positions -> [B, D] (dropout is the caller's)."""
    _host_only(chars, conv1.weight)
    signal = nn.functional.one_hot(chars, num_chars).transpose(1, 2).float()      # [B, C, L]
    for conv in (conv1, conv2):
        signal = nn.functional.relu(conv(signal))                                  # [B, F, positions left]
    return torch.max(conv3(signal), dim=-1)[0]
