#!/usr/bin/env python
"""Generate the EGC golden fixtures tests/golden/egc_*.npz from the REAL reference's `EGCMessagePassingLayer`
(egcmessagepassing.py), imported unmodified and executed on CPU in fp32 -- like make_golden.py, whose graph helpers
it reuses, with the same shims (oracle/shims.py: torch_scatter restated, dpu_utils stubbed).

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_egc.py

Every layer fixture stores: x, the adjacency lists, the layer's initial state_dict under `seed` (keys `state.<reference
key>`), its output y and -- for a fixed upstream gradient gout of the scalar loss sum(y * gout) -- the gradients of x
(`grad.x`) and of every parameter (`grad.<reference key>`).  egc_stack stores a reference GraphNeuralNetwork forward
([residual origin, EGC, EGC, MeanResidualLayer]) with both layers' states under `l0.` / `l1.`.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from ptgnn.neuralmodels.gnn import GraphNeuralNetwork  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing import MeanResidualLayer  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing.egcmessagepassing import EGCMessagePassingLayer  # noqa: E402

from oracle.fixtures import pack_adj  # noqa: E402

# name, aggregation, H_in, heads K, bases B, head dim Dh, seed
LAYERS = [
    ("egc_sum_k8b4d8", "sum", 24, 8, 4, 8, 11),
    ("egc_mean_k8b4d16", "mean", 32, 8, 4, 16, 12),
    ("egc_max_k4b2d32", "max", 48, 4, 2, 32, 13),
    ("egc_min_k3b3d12", "min", 20, 3, 3, 12, 14),
    ("egc_max_k8b4d16", "max", 64, 8, 4, 16, 15),
]


def state_arrays(prefix, module):
    return {prefix + k: v.detach().clone() for k, v in module.state_dict().items()}


def layer_fixtures():
    gen = torch.Generator().manual_seed(2468)
    n = 40
    for name, agg, H, K, B, Dh, seed in LAYERS:
        D = K * Dh
        adj = G.tricky_adj(gen, n)
        x = torch.randn(n, H, generator=gen)
        gout = torch.randn(n, D, generator=gen)
        torch.manual_seed(seed)
        layer = EGCMessagePassingLayer(H, D, len(adj), agg, num_bases=B, num_heads=K)
        state = state_arrays("state.", layer)
        xr = x.clone().requires_grad_(True)
        y = layer(xr, adj, torch.zeros(n, dtype=torch.int64), {}, {}, G.empty_feats(adj))
        (y * gout).sum().backward()
        grads = {"grad.x": xr.grad}
        grads.update({"grad." + k: p.grad for k, p in layer.named_parameters()})
        G.save(name, x=x, y=y.detach(), gout=gout, **pack_adj(adj), **state, **grads,
               meta=np.asarray([H, D, len(adj), K, B, seed]), agg=np.asarray(agg))


def stack_fixture():
    gen = torch.Generator().manual_seed(1357)
    n, H = 60, 32
    node_to_graph = torch.repeat_interleave(torch.arange(3), 20)
    adj = G.rand_adj(gen, n, [90, 0, 45])
    x = torch.randn(n, H, generator=gen)
    T = 2 * len(adj) + 1        # backwards edges + self edges
    torch.manual_seed(21)
    e0 = EGCMessagePassingLayer(H, H, T, "sum", num_bases=4, num_heads=8)
    e1 = EGCMessagePassingLayer(H, H, T, "max", num_bases=2, num_heads=4)
    r = MeanResidualLayer(H)
    net = GraphNeuralNetwork([r.pass_through_dummy_layer(), e0, e1, r], G._Identity(), introduce_backwards_edges=True,
                             add_self_edges=True).eval()
    with torch.no_grad():
        out = net(node_data={"x": x}, adjacency_lists=list(adj), edge_feature_data=[], node_to_graph_idx=node_to_graph,
                  reference_node_ids={}, reference_node_graph_idx={}, num_graphs=3)
    G.save("egc_stack", x=x, y=out.output_node_representations, node_to_graph_idx=node_to_graph, **pack_adj(adj),
           **state_arrays("l0.", e0), **state_arrays("l1.", e1),
           num_edges=np.asarray(net.report_metrics()["num_edges"]))


if __name__ == "__main__":
    torch.set_num_threads(1)
    layer_fixtures()
    stack_fixture()
