#!/usr/bin/env python
"""Generate the PNA golden fixtures tests/golden/pna_*.npz from the REAL reference's `MlpMessagePassingLayer` with
`PnaMessageAggregation` (mlpmessagepassing.py, pna_aggregation.py), imported unmodified and executed on CPU in fp32 --
like make_golden.py, whose graph helpers it reuses, with the same shims (oracle/shims.py: torch_scatter restated,
dpu_utils stubbed).

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_pna.py

Every graph has zero-in-degree nodes, degree-1 rows, duplicate edges (equal messages: max / min ties), an empty edge
type and one destination with 300 in-edges (a row beyond the 256 in-edges that one lane group folds).
Layer fixtures store: x, the adjacency lists, the layer's initial state_dict under `seed` (keys `state.<reference key>`),
its output y and -- for a fixed upstream gradient gout of the scalar loss sum(y * gout) -- the gradients of x (`grad.x`)
and of every parameter (`grad.<reference key>`).  pna_module stores the aggregation module alone (messages, unsorted
targets, num_nodes beyond the largest target -> out and the messages' gradient; no max / min ties: oracle/scatter_ref.py
spreads a tied max / min gradient over the tied elements where torch_scatter picks one, so per-message tie gradients
are tested against the documented rule instead, tests/test_gpu_pna.py); pna_stack a reference
GraphNeuralNetwork forward ([residual origin, MLP-PNA, MLP-PNA, MeanResidualLayer]) with the layers' states under
`l0.` / `l1.`.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from ptgnn.neuralmodels.gnn import GraphNeuralNetwork  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing import MeanResidualLayer, MlpMessagePassingLayer  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing.pna_aggregation import PnaMessageAggregation  # noqa: E402

from oracle.fixtures import pack_adj  # noqa: E402

HUB_DEGREE = 300

# name, H_in, message dim M, output dim, delta, constructor keywords, seed
LAYERS = [
    ("pna_target_m8", 16, 8, 16, 1, {}, 31),
    ("pna_hidden1_m8", 16, 8, 16, 1, dict(mlp_hidden_layers=1), 32),
    ("pna_delta25_m8", 16, 8, 12, 2.5, {}, 33),
    ("pna_noln_nodense_m8", 16, 8, 16, 1, dict(use_layer_norm=False, use_dense_layer=False), 34),
    ("pna_target_m6", 12, 6, 16, 1, {}, 35),
    ("pna_notarget_m32", 32, 32, 32, 1, dict(use_target_state_as_message_input=False), 36),
    ("pna_target_m32", 32, 32, 32, 1.5, {}, 37),
]


def pna_adj(gen, n):
    """3 edge types: random edges with duplicates (1 -> 2 three times, 4 -> 4 twice); EMPTY type; a hub destination 3
    with HUB_DEGREE in-edges.  Nodes n-1 and n-2 never receive an edge."""
    a0 = G.rand_adj(gen, n - 2, [2 * n])[0]
    a0 = (torch.cat([a0[0], torch.tensor([1, 1, 1, 4, 4])]), torch.cat([a0[1], torch.tensor([2, 2, 2, 4, 4])]))
    a1 = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    hub_src = torch.randint(0, n, (HUB_DEGREE,), generator=gen, dtype=torch.int64)
    a2 = (hub_src, torch.full((HUB_DEGREE,), 3, dtype=torch.int64))
    return [a0, a1, a2]


def state_arrays(prefix, module):
    return {prefix + k: v.detach().clone() for k, v in module.state_dict().items()}


def layer_fixtures():
    gen = torch.Generator().manual_seed(97531)
    n = 40
    for name, H, M, D, delta, kw, seed in LAYERS:
        adj = pna_adj(gen, n)
        x = torch.randn(n, H, generator=gen)
        gout = torch.randn(n, D if kw.get("use_dense_layer", True) else 15 * M, generator=gen)
        torch.manual_seed(seed)
        layer = MlpMessagePassingLayer(H, D, M, len(adj), PnaMessageAggregation(delta=delta), **kw)
        state = state_arrays("state.", layer)
        xr = x.clone().requires_grad_(True)
        y = layer(xr, adj, torch.zeros(n, dtype=torch.int64), {}, {}, G.empty_feats(adj))
        (y * gout).sum().backward()
        grads = {"grad.x": xr.grad}
        grads.update({"grad." + k: p.grad for k, p in layer.named_parameters()})
        flags = [kw.get("mlp_hidden_layers", 0), int(kw.get("use_target_state_as_message_input", True)),
                 int(kw.get("use_layer_norm", True)), int(kw.get("use_dense_layer", True))]
        G.save(name, x=x, y=y.detach(), gout=gout, **pack_adj(adj), **state, **grads,
               meta=np.asarray([H, M, D, len(adj)] + flags + [seed]), delta=np.asarray(float(delta)))


def module_fixture():
    gen = torch.Generator().manual_seed(8642)
    num_nodes, M = 50, 8                           # targets stay below 44: rows 44..49 are empty
    t = torch.randint(0, 44, (120,), generator=gen)
    t = torch.cat([t, torch.full((HUB_DEGREE,), 7, dtype=torch.int64)])
    msgs = torch.randn(t.shape[0], M, generator=gen)
    perm = torch.randperm(t.shape[0], generator=gen)
    t, msgs = t[perm], msgs[perm]                   # unsorted targets
    gout = torch.randn(num_nodes, 15 * M, generator=gen)
    agg = PnaMessageAggregation(delta=1)
    mr = msgs.clone().requires_grad_(True)
    out = agg(messages=mr, message_targets=t, num_nodes=num_nodes)
    (out * gout).sum().backward()
    G.save("pna_module", messages=msgs, targets=t, num_nodes=np.asarray(num_nodes), out=out.detach(), gout=gout,
           grad=mr.grad, delta=np.asarray(1.0))


def stack_fixture():
    gen = torch.Generator().manual_seed(2468)
    n, H = 60, 32
    node_to_graph = torch.repeat_interleave(torch.arange(3), 20)
    adj = G.rand_adj(gen, n, [90, 0, 45])
    x = torch.randn(n, H, generator=gen)
    T = 2 * len(adj) + 1        # backwards edges + self edges
    torch.manual_seed(41)
    l0 = MlpMessagePassingLayer(H, H, 8, T, PnaMessageAggregation())
    l1 = MlpMessagePassingLayer(H, H, 32, T, PnaMessageAggregation(delta=2.0), use_target_state_as_message_input=False)
    r = MeanResidualLayer(H)
    net = GraphNeuralNetwork([r.pass_through_dummy_layer(), l0, l1, r], G._Identity(), introduce_backwards_edges=True,
                             add_self_edges=True).eval()
    with torch.no_grad():
        out = net(node_data={"x": x}, adjacency_lists=list(adj), edge_feature_data=[], node_to_graph_idx=node_to_graph,
                  reference_node_ids={}, reference_node_graph_idx={}, num_graphs=3)
    G.save("pna_stack", x=x, y=out.output_node_representations, node_to_graph_idx=node_to_graph, **pack_adj(adj),
           **state_arrays("l0.", l0), **state_arrays("l1.", l1), num_edges=np.asarray(net.report_metrics()["num_edges"]))


if __name__ == "__main__":
    torch.set_num_threads(1)
    layer_fixtures()
    module_fixture()
    stack_fixture()
