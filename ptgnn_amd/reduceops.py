"""Node -> graph pooling ("var-sized element reduce") and the global-exchange layer that uses it:
mirrors of ptgnn/neuralmodels/reduceops/varsizedsummary.py:11-41,67-178 and
ptgnn/neuralmodels/gnn/messagepassing/globalgraphexchange.py (same class names, constructor keywords
and name-mangled parameter names), used by the VarMisuse GGNN stack (varmisuse/train.py:76-107).

The pooling is the same segment reduce as message aggregation with `node_to_graph_idx` as the index.
A disjoint-union batch lists the nodes of graph 0, then graph 1, ... (graphneuralnetwork.py:418-423),
so the index is SORTED and the plan needs no sort at all: rowptr = searchsorted, col = identity.
"""
import math
from typing import NamedTuple, Optional, Union

import torch
from torch import nn

from ptgnn_amd import _lib, dense, ops, scatter as scatter_facade, torch_route
from ptgnn_amd.layers import (AbstractMessagePassingLayer, _check_device, _index_plan, _no_grad_needed,  # noqa: F401
                              _num_samples)
from ptgnn_amd.scatter import gather_rows as gather_rows_autograd, segment_reduce


class ElementsToSummaryRepresentationInput(NamedTuple):
    """varsizedsummary.py:11-18."""
    element_embeddings: torch.Tensor
    element_to_sample_map: torch.Tensor
    num_samples: Union[torch.Tensor, int]


class AbstractVarSizedElementReduce(nn.Module):
    def forward(self, inputs: ElementsToSummaryRepresentationInput) -> torch.Tensor:
        raise NotImplementedError


def _pool(values: torch.Tensor, index: torch.Tensor, num_samples, reduce: str) -> torch.Tensor:
    if not values.is_cuda:    # device dispatch: CPU tensors take the plain-torch route (ptgnn_amd/torch_route.py)
        return torch_route.segment(values, index, int(num_samples), reduce)    # varsizedsummary.py:35-41: no dtype cast
    plan = _index_plan(index, int(num_samples))
    dt = values.dtype
    return segment_reduce(values.to(torch.float32).contiguous(), plan, reduce).to(dt)


class SimpleVarSizedElementReduce(AbstractVarSizedElementReduce):
    def __init__(self, summarization_type: str):
        super().__init__()
        assert summarization_type in {"sum", "mean", "max", "min"}
        self.__summarization_type = summarization_type

    @property
    def summarization_type(self) -> str:
        return self.__summarization_type

    def forward(self, inputs: ElementsToSummaryRepresentationInput) -> torch.Tensor:
        return _pool(inputs.element_embeddings, inputs.element_to_sample_map, inputs.num_samples,
                     self.__summarization_type)


class _WeightedPool(torch.autograd.Function):
    """sum_{i in sample} sigmoid(x_i . w) x_i as ONE node: forward and backward are the two HIP entry points of
    csrc/weighted_pool.hip (no gemv, no [N, D] product in memory, deterministic weight gradient)."""

    @staticmethod
    def forward(ctx, x, w, index, plan):
        ctx.save_for_backward(x, w, index)
        return ops.weighted_pool(x, w, plan)

    @staticmethod
    def backward(ctx, grad_out):
        x, w, index = ctx.saved_tensors
        gx, gw = ops.weighted_pool_backward(x, w, index, grad_out.contiguous())
        return gx, gw.reshape(w.shape), None, None


class WeightedSumVarSizedElementReduce(AbstractVarSizedElementReduce):
    def __init__(self, representation_size: int):
        super().__init__()
        self.__weights_layer = nn.Linear(representation_size, 1, bias=False)

    @property
    def score_weight(self) -> torch.Tensor:
        """[1, D] weight of the scoring Linear (varsizedsummary.py:71)."""
        return self.__weights_layer.weight

    def forward(self, inputs: ElementsToSummaryRepresentationInput) -> torch.Tensor:
        x, index = inputs.element_embeddings, inputs.element_to_sample_map
        w = self.__weights_layer.weight
        if not x.is_cuda:      # device dispatch: the reference's own operator sequence (varsizedsummary.py:73-81)
            weights = torch.sigmoid(self.__weights_layer(x).squeeze(-1))          # [num_elements]
            return _pool(x * weights.unsqueeze(-1), index, inputs.num_samples, "sum")
        # GPU: score, scaling and segment sum in one HIP pass (csrc/weighted_pool.hip); fp16 / bf16 states (AMP) are
        # pooled in fp32 and cast back, like every aggregation of the package
        plan = _index_plan(index, int(inputs.num_samples))
        dt = x.dtype
        xf, wf = x.to(torch.float32), w.to(torch.float32)
        if _no_grad_needed(xf, wf):
            return ops.weighted_pool(xf, wf, plan).to(dt)
        return _WeightedPool.apply(xf, wf, index, plan).to(dt)


class _AttentionPool(torch.autograd.Function):
    """P[g,h] = sum_{i in g} softmax_g(u[g,h] . x_i) x_i over the plan of the element -> sample map as ONE node: forward
    and backward are the two passes of csrc/attention_pool.hip (no [N, heads * D] tensor, deterministic grad_u)."""

    @staticmethod
    def forward(ctx, x, u, plan):
        pooled, stats = ops.attention_pool(x, u, plan)
        ctx.plan = plan
        ctx.save_for_backward(x, u, pooled, stats)
        return pooled

    @staticmethod
    def backward(ctx, grad):
        x, u, pooled, stats = ctx.saved_tensors
        gx, gu = ops.attention_pool_backward(x, u, ctx.plan, pooled, stats, grad.contiguous())
        return gx, gu, None


class _HeadExpand(torch.autograd.Function):
    """u[g,h] = scale * W[h-block]^T q[g, h-block] (ops.head_expand); backward: dq = head_contract(du, W),
    dW = head_weight_grad(q, du)."""

    @staticmethod
    def forward(ctx, a, w, num_heads, scale):
        ctx.save_for_backward(a, w)
        ctx.num_heads, ctx.scale = num_heads, scale
        return ops.head_expand(a, w, num_heads, scale)

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        g = g.contiguous()
        da = ops.head_contract(g, w, ctx.num_heads, ctx.scale) if ctx.needs_input_grad[0] else None
        dw = ops.head_weight_grad(a, g, ctx.num_heads, ctx.scale) if ctx.needs_input_grad[1] else None
        return da, dw, None, None


class _HeadContract(torch.autograd.Function):
    """v[g, h-block] = W[h-block] P[g,h] (ops.head_contract: the value Linear on the pools); backward:
    dP = head_expand(dv, W), dW = head_weight_grad(dv, P)."""

    @staticmethod
    def forward(ctx, b, w, num_heads):
        ctx.save_for_backward(b, w)
        ctx.num_heads = num_heads
        return ops.head_contract(b, w, num_heads)

    @staticmethod
    def backward(ctx, g):
        b, w = ctx.saved_tensors
        g = g.contiguous()
        db = ops.head_expand(g, w, ctx.num_heads) if ctx.needs_input_grad[0] else None
        dw = ops.head_weight_grad(g, b, ctx.num_heads) if ctx.needs_input_grad[1] else None
        return db, dw, None


def _composed_attention_summary(x, index, plan, num_samples: int, queries, key_weight, value_weight, output_weight,
                                num_heads: int, single_head: bool) -> torch.Tensor:
    """Shapes beyond the fused pool (more than 8 heads, D > 1024): the reference's operator sequence on the package's
    other HIP entry points -- dense.linear, the row gather, the facade's segment log-softmax and segment sums."""
    n, hidden = x.shape[0], key_weight.shape[0]
    keys = dense.linear(x, key_weight)                                            # [N, hidden]
    queries_all = gather_rows_autograd(queries.contiguous(), index, plan)          # [N, hidden]
    if single_head:
        scores = (queries_all * keys).sum(-1)
    else:
        dk = hidden // num_heads
        scores = (queries_all * keys).reshape(n, num_heads, dk).sum(-1) / math.sqrt(dk)
    probs = scatter_facade.scatter_log_softmax(scores, index, dim=0, eps=0.0, dim_size=num_samples).exp()
    if single_head:
        return scatter_facade.scatter_sum(dense.linear(x, output_weight) * probs.unsqueeze(-1), index, dim=0,
                                          dim_size=num_samples)
    if value_weight is not None:
        rows = probs.unsqueeze(-1) * dense.linear(x, value_weight).reshape(n, num_heads, hidden // num_heads)
    else:
        rows = probs.unsqueeze(-1) * x.unsqueeze(1)
    per_sample = scatter_facade.scatter_sum(rows.reshape(n, -1), index, dim=0, dim_size=num_samples)
    return dense.linear(per_sample, output_weight)


def _attention_summary(inputs, queries: torch.Tensor, key_weight: torch.Tensor, value_weight: Optional[torch.Tensor],
                       output_weight: torch.Tensor, num_heads: int, single_head: bool) -> torch.Tensor:
    """The attention reducers after their query summariser.  GPU: u = c * blockdiag(q) W_k on the samples, the softmax
    pool in one HIP pass over the elements, the value / output Linears on the [G, ...] pools (csrc/attention_pool.hip
    header); fp16 / bf16 elements are pooled in fp32 and cast back."""
    x, index = inputs.element_embeddings, inputs.element_to_sample_map
    G = int(inputs.num_samples)
    if not x.is_cuda:       # device dispatch: the reference's own operator sequence
        return torch_route.attention_summary(x, index, G, queries, key_weight, value_weight, output_weight, num_heads,
                                             single_head)
    dt = x.dtype
    xf, q = x.to(torch.float32), queries.to(torch.float32)
    wk, wo = key_weight.to(torch.float32), output_weight.to(torch.float32)
    wv = value_weight.to(torch.float32) if value_weight is not None else None
    plan = _index_plan(index, G)
    hidden, D = wk.shape
    if not ops.attention_pool_supported(D, num_heads):
        return _composed_attention_summary(xf, index, plan, G, q, wk, wv, wo, num_heads, single_head).to(dt)
    scale = 1.0 if single_head else 1.0 / math.sqrt(hidden // num_heads)
    u = _HeadExpand.apply(q.contiguous(), wk, num_heads, scale)                 # [G, heads, D]
    pooled = _AttentionPool.apply(xf, u, plan)                                  # [G, heads, D]
    if wv is not None:
        pooled = _HeadContract.apply(pooled, wv, num_heads)                     # [G, hidden]
    return dense.linear(pooled.reshape(G, -1), wo).to(dt)


class SelfAttentionVarSizedElementReduce(AbstractVarSizedElementReduce):
    """varsizedsummary.py:84-113 (same constructor keywords, submodule order and name-mangled parameter names)."""

    def __init__(self, input_representation_size: int, hidden_size: int, output_representation_size: int,
                 query_representation_summarizer: AbstractVarSizedElementReduce):
        super().__init__()
        self.__query_layer = query_representation_summarizer
        self.__key_layer = nn.Linear(input_representation_size, hidden_size, bias=False)
        self.__output_layer = nn.Linear(input_representation_size, output_representation_size, bias=False)

    def forward(self, inputs: ElementsToSummaryRepresentationInput) -> torch.Tensor:
        queries = self.__query_layer(inputs)                                     # [num_samples, hidden]
        return _attention_summary(inputs, queries, self.__key_layer.weight, None, self.__output_layer.weight, 1, True)


class MultiheadSelfAttentionVarSizedElementReduce(AbstractVarSizedElementReduce):
    """varsizedsummary.py:116-178 (same constructor keywords, submodule order and name-mangled parameter names); the
    summariser of the Graph2Seq task (graph2seq/graph2seq.py:116-122)."""

    def __init__(self, input_representation_size: int, hidden_size: int, output_representation_size: int,
                 num_heads: int, query_representation_summarizer: AbstractVarSizedElementReduce,
                 use_value_layer: bool = False):
        super().__init__()
        self.__query_layer = query_representation_summarizer
        self.__key_layer = nn.Linear(input_representation_size, hidden_size, bias=False)
        assert hidden_size % num_heads == 0, "Hidden size must be divisible by the number of heads."
        self.__use_value_layer = use_value_layer
        if use_value_layer:
            self.__value_layer = nn.Linear(input_representation_size, hidden_size, bias=False)
            self.__output_layer = nn.Linear(hidden_size, output_representation_size, bias=False)
        else:
            self.__output_layer = nn.Linear(input_representation_size * num_heads, output_representation_size,
                                            bias=False)
        self.__num_heads = num_heads

    def forward(self, inputs: ElementsToSummaryRepresentationInput) -> torch.Tensor:
        queries = self.__query_layer(inputs)                                     # [num_samples, hidden]
        value_weight = self.__value_layer.weight if self.__use_value_layer else None
        return _attention_summary(inputs, queries, self.__key_layer.weight, value_weight, self.__output_layer.weight,
                                  self.__num_heads, False)


class AbstractGlobalGraphExchange(AbstractMessagePassingLayer):
    """globalgraphexchange.py:13-45: pool node states per graph, broadcast back, update the nodes."""

    def __init__(self, global_graph_representation_module: AbstractVarSizedElementReduce,
                 dropout_rate: float = 0.0):
        super().__init__()
        self.__global_graph_representation_module = global_graph_representation_module
        self.__dropout = nn.Dropout(p=dropout_rate)

    def _update_node_states(self, node_states, global_info_per_node):
        raise NotImplementedError

    @property
    def pooling_module(self) -> AbstractVarSizedElementReduce:
        return self.__global_graph_representation_module

    def forward(self, node_states, adjacency_lists, node_to_graph_idx, reference_node_ids,
                reference_node_graph_idx, edge_features) -> torch.Tensor:
        if not node_states.is_cuda:   # globalgraphexchange.py:37-45 on host tensors
            num_graphs = _num_samples(node_to_graph_idx)
            e = ElementsToSummaryRepresentationInput(node_states, node_to_graph_idx, num_graphs)
            graph_reps = self.__dropout(self.__global_graph_representation_module(e))
            return self._update_node_states(node_states, graph_reps[node_to_graph_idx])
        if node_states.dtype in (torch.float16, torch.bfloat16):   # AMP: fp32 inside, caller's dtype outside
            return self.forward(node_states.float(), adjacency_lists, node_to_graph_idx, reference_node_ids,
                                reference_node_graph_idx, edge_features).to(node_states.dtype)
        num_graphs = _num_samples(node_to_graph_idx)
        e = ElementsToSummaryRepresentationInput(node_states, node_to_graph_idx, num_graphs)
        graph_reps = self.__dropout(self.__global_graph_representation_module(e))
        if graph_reps.dtype != torch.float32:
            per_node = graph_reps[node_to_graph_idx]
        elif _no_grad_needed(graph_reps):
            per_node = ops.gather_rows(graph_reps.contiguous(), node_to_graph_idx)
        else:   # training: HIP row gather whose backward is the HIP segment-sum over the graphs (deterministic)
            plan = _index_plan(node_to_graph_idx, num_graphs)
            per_node = gather_rows_autograd(graph_reps.contiguous(), node_to_graph_idx, plan)
        return self._update_node_states(node_states, per_node)

    def forward_sharded(self, node_states, shard) -> torch.Tensor:
        """The same exchange over a dst-range shard (ptgnn_amd/sharded.py): every rank pools ITS nodes per graph,
        the [num_graphs, D] partial pools are combined with one small all-reduce (a graph may straddle a rank
        boundary), and the broadcast back + node update are local."""
        from ptgnn_amd import sharded
        _check_device(node_states)
        idx, G = shard.node_to_graph_idx, shard.num_graphs
        if idx is None:
            raise _lib.PtgnnAmdError("forward_sharded of a global-exchange layer needs "
                                     "ShardedGraph.attach_graph_index(node_to_graph_idx_local, num_graphs)")
        pool = self.__global_graph_representation_module
        if isinstance(pool, WeightedSumVarSizedElementReduce):
            kind, local = "sum", pool(ElementsToSummaryRepresentationInput(node_states, idx, G))
        elif isinstance(pool, SimpleVarSizedElementReduce):
            kind = pool.summarization_type
            local = _pool(node_states, idx, G, "sum" if kind == "mean" else kind)
        else:
            raise _lib.PtgnnAmdError(f"forward_sharded: cannot combine partial pools of {type(pool).__name__}")
        counts = torch.bincount(idx, minlength=G)[:G]
        graph_reps = sharded.combine_graph_pools(local, counts, kind, shard.group)
        p = self.__dropout.p if self.training else 0.0
        if p > 0 and shard.world > 1:
            # the unsharded layer draws ONE dropout mask per graph representation (globalgraphexchange.py:44-46); every
            # rank holds the same combined representations, so the mask must be the same on every rank too: rank 0 of
            # the group draws it, one small broadcast ([num_graphs, D]) carries it
            import torch.distributed as dist
            keep = (torch.rand_like(graph_reps) >= p).to(graph_reps.dtype) / (1.0 - p)
            dist.broadcast(keep, src=dist.get_global_rank(shard.group, 0) if shard.group is not None else 0,
                           group=shard.group)
            graph_reps = graph_reps * keep
        else:
            graph_reps = self.__dropout(graph_reps)
        if _no_grad_needed(graph_reps):
            per_node = ops.gather_rows(graph_reps.contiguous(), idx)
        else:
            per_node = gather_rows_autograd(graph_reps.contiguous(), idx, _index_plan(idx, G))
        return self._update_node_states(node_states, per_node)


class GruGlobalStateUpdate(AbstractGlobalGraphExchange):
    def __init__(self, global_graph_representation_module: AbstractVarSizedElementReduce,
                 input_state_size: int, summarized_state_size: int, dropout_rate: float = 0.0):
        super().__init__(global_graph_representation_module, dropout_rate)
        self.__input_dim = input_state_size
        self.__summarized_state_size = summarized_state_size
        self.__gru_cell = nn.GRUCell(input_size=summarized_state_size, hidden_size=input_state_size)

    def _update_node_states(self, node_states, global_info_per_node):
        gru = self.__gru_cell
        if not node_states.is_cuda:
            return gru(global_info_per_node, node_states)
        if (node_states.dtype == torch.float32
                and _no_grad_needed(node_states, global_info_per_node, *gru.parameters())):
            return ops.gru_cell(global_info_per_node, node_states, gru.weight_ih, gru.weight_hh,
                                gru.bias_ih, gru.bias_hh)
        return dense.gru_cell(gru, global_info_per_node, node_states)

    @property
    def input_state_dimension(self) -> int:
        return self.__input_dim

    @property
    def output_state_dimension(self) -> int:
        return self.__input_dim

    def export_weights(self) -> dict:
        """Weights in the layout the parity oracle consumes (tests only read this)."""
        gru, pool = self.__gru_cell, self.pooling_module
        spec = {"kind": "global_gru", "w_ih": gru.weight_ih.detach().cpu(), "w_hh": gru.weight_hh.detach().cpu(),
                "b_ih": gru.bias_ih.detach().cpu(), "b_hh": gru.bias_hh.detach().cpu()}
        if isinstance(pool, WeightedSumVarSizedElementReduce):
            spec.update(pool="weighted_sum", pool_w=pool.score_weight.detach().cpu())
        else:
            spec["pool"] = pool.summarization_type
        return spec
