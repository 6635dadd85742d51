"""EGCMessagePassingLayer on host tensors (ptgnn_amd.torch_route.egc_layer) against fixtures of the reference's own
class (tests/golden/make_golden_egc.py): state_dict keys, initial parameters, outputs, gradients, the GNN container,
and the sharded form refusing the layer."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle.fixtures import unpack_adj
from ptgnn_amd import PtgnnAmdError
from ptgnn_amd.layers import EGCMessagePassingLayer, MeanResidualLayer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYER_FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLDEN, "egc_*.npz")) if not f.endswith("egc_stack.npz"))
TOL = 1e-6


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def prefixed(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}


def make_layer(fx, seed=None):
    H, D, T, K, B, s = (int(v) for v in fx["meta"])
    if seed is not None:
        torch.manual_seed(s)
    return EGCMessagePassingLayer(H, D, T, str(fx["agg"]), num_bases=B, num_heads=K)


def run(layer, fx, x):
    adj = unpack_adj(fx)
    feats = [torch.empty(s.shape[0], 0) for s, _ in adj]
    return layer(x, adj, torch.zeros(x.shape[0], dtype=torch.int64), {}, {}, feats)


def test_fixtures_present():
    assert len(LAYER_FIXTURES) >= 5
    aggs = {str(load(f)["agg"]) for f in LAYER_FIXTURES}
    assert aggs == {"sum", "mean", "max", "min"}


@pytest.mark.parametrize("path", LAYER_FIXTURES, ids=os.path.basename)
def test_state_dict_loads_strict_and_initial_parameters_match(path):
    fx = load(path)
    state = prefixed(fx, "state.")
    assert set(state) == {f"_EGCMessagePassingLayer__bases.{t}.weight" for t in range(int(fx["meta"][2]))} | {
        "_EGCMessagePassingLayer__weight_coeffs.weight", "_EGCMessagePassingLayer__weight_coeffs.bias"}
    layer = make_layer(fx, seed=True)            # same seed, same construction order as the reference
    for k, v in layer.state_dict().items():
        assert torch.equal(v, state[k]), k
    fresh = make_layer(fx)
    fresh.load_state_dict(state, strict=True)


@pytest.mark.parametrize("path", LAYER_FIXTURES, ids=os.path.basename)
def test_cpu_route_output_and_gradients(path):
    fx = load(path)
    layer = make_layer(fx)
    layer.load_state_dict(prefixed(fx, "state."), strict=True)
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    y = run(layer, fx, x)
    assert layer.input_state_dimension == x.shape[1] and layer.output_state_dimension == y.shape[1]
    assert float((y.detach() - torch.from_numpy(fx["y"])).abs().max()) <= TOL
    (y * torch.from_numpy(fx["gout"])).sum().backward()
    assert float((x.grad - torch.from_numpy(fx["grad.x"])).abs().max()) <= 1e-5
    for k, p in layer.named_parameters():
        want = torch.from_numpy(fx["grad." + k])
        assert float((p.grad - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), k


def test_cpu_stack_matches_reference_container():
    from ptgnn_amd.gnn import GraphNeuralNetwork
    fx = load(os.path.join(GOLDEN, "egc_stack.npz"))
    x = torch.from_numpy(fx["x"])
    H = x.shape[1]
    T = 2 * int(fx["__num_edge_types__"]) + 1
    e0 = EGCMessagePassingLayer(H, H, T, "sum", num_bases=4, num_heads=8)
    e1 = EGCMessagePassingLayer(H, H, T, "max", num_bases=2, num_heads=4)
    e0.load_state_dict(prefixed(fx, "l0."), strict=True)
    e1.load_state_dict(prefixed(fx, "l1."), strict=True)
    r = MeanResidualLayer(H)
    net = GraphNeuralNetwork([r.pass_through_dummy_layer(), e0, e1, r], torch.nn.Identity(),
                             introduce_backwards_edges=True, add_self_edges=True).eval()
    with torch.no_grad():
        out = net(node_data={"input": x}, adjacency_lists=unpack_adj(fx), edge_feature_data=[],
                  node_to_graph_idx=torch.from_numpy(fx["node_to_graph_idx"]), reference_node_ids={},
                  reference_node_graph_idx={}, num_graphs=3)
    assert float((out.output_node_representations - torch.from_numpy(fx["y"])).abs().max()) <= TOL


def test_forward_sharded_raises():
    layer = EGCMessagePassingLayer(16, 16, 2, "sum", num_bases=2, num_heads=4)
    with pytest.raises(PtgnnAmdError, match="not supported under dst-range sharding"):
        layer.forward_sharded(torch.zeros(4, 16), shard=None)
