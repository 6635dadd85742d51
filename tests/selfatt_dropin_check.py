"""Executed in a FRESH interpreter by tests/test_selfatt_cpu.py (the reference must be importable before
ptgnn_amd.layers is first imported, so that the layers subclass the reference's ABC) -- the pattern of
tests/dropin_check.py, for MultiHeadSelfAttentionMessagePassing:

  * ptgnn_amd.layers.MultiHeadSelfAttentionMessagePassing and the reference's class (selfattmessagepassing.py:9-136)
    exchange state_dicts, strict, both ways;
  * (gradients: with autograd running through the reference's attention, which its window generator switches off)
  * inside the reference's own GraphNeuralNetwork container, between two GGNN layers, on a batch of the reference's own
    batcher on the CPU, the two agree on the output and on every parameter gradient to 1e-6.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import shims  # noqa: E402

shims.install()
from ptgnn.baseneuralmodel import AbstractNeuralModel  # noqa: E402
from ptgnn.neuralmodels.gnn import GraphData, GraphNeuralNetwork, GraphNeuralNetworkModel  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing import GatedMessagePassingLayer  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing.abstractmessagepassing import AbstractMessagePassingLayer  # noqa: E402
from ptgnn.neuralmodels.gnn.messagepassing.selfattmessagepassing import (  # noqa: E402
    MultiHeadSelfAttentionMessagePassing as RefSelfAtt)

from ptgnn.neuralmodels.gnn.messagepassing import selfattmessagepassing as ref_module  # noqa: E402

from ptgnn_amd import layers as L  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from selfatt_cases import differentiable_reference  # noqa: E402

assert issubclass(L.MultiHeadSelfAttentionMessagePassing, AbstractMessagePassingLayer)
SELFATT = dict(key_query_dimension=5, value_dimension=7, output_dimension=16, intermediate_dimension=24, num_heads=3,
               max_num_nodes=7)     # graphs of 9 .. 18 nodes: two or three windows each
H = 16
TOL = 1e-6


class _Identity(torch.nn.Module):
    def forward(self, x):
        return x


class _NodeModel(AbstractNeuralModel):
    def initialize_metadata(self): pass
    def update_metadata_from(self, datapoint): pass
    def finalize_metadata(self): pass
    def build_neural_module(self): return _Identity()
    def tensorize(self, datapoint): return int(datapoint)
    def initialize_minibatch(self): return {"ids": []}

    def extend_minibatch_with(self, tensorized_datapoint, partial_minibatch):
        partial_minibatch["ids"].append(tensorized_datapoint)
        return True

    def finalize_minibatch(self, accumulated_minibatch_data, device):
        g = torch.Generator().manual_seed(len(accumulated_minibatch_data["ids"]))
        return {"x": torch.randn(len(accumulated_minibatch_data["ids"]), H, generator=g)}


def ref_layers(n):
    return [GatedMessagePassingLayer(H, 24, n, "max"), RefSelfAtt(H, **SELFATT),
            GatedMessagePassingLayer(H, H, n, "mean")]


def our_layers(n):
    return [L.GatedMessagePassingLayer(H, 24, n, "max"), L.MultiHeadSelfAttentionMessagePassing(H, **SELFATT),
            L.GatedMessagePassingLayer(H, H, n, "mean")]


def make_model(creator):
    m = GraphNeuralNetworkModel(node_representation_model=_NodeModel(), message_passing_layer_creator=creator,
                                stop_extending_minibatch_after_num_nodes=500, add_self_edges=True)
    rng = np.random.RandomState(3)
    graphs = []
    for g in range(4):
        n = 1 if g == 2 else 9 + 3 * g                                # a one-node graph among the others
        edges = {"a": [(int(a), int(b)) for a, b in rng.randint(0, n, (2 * n, 2))],
                 "b": [(int(a), int(b)) for a, b in rng.randint(0, n, (n // 2, 2))]}
        graphs.append(GraphData(node_information=list(range(n)), edges=edges, reference_nodes={"r": [0, n - 1]}))
    m.compute_metadata(iter(graphs), parallelize=False)
    return m, graphs


ref_model, graphs = make_model(ref_layers)
our_model, _ = make_model(our_layers)
torch.manual_seed(11)
ref_net = ref_model.build_neural_module()
our_net = our_model.build_neural_module()
assert type(our_net) is GraphNeuralNetwork                      # the REFERENCE's container, our layers inside

ref_att = [m for m in ref_net.modules() if isinstance(m, RefSelfAtt)]
our_att = [m for m in our_net.modules() if isinstance(m, L.MultiHeadSelfAttentionMessagePassing)]
assert len(ref_att) == 1 and len(our_att) == 1
ref_att, our_att = ref_att[0], our_att[0]
assert list(our_att.state_dict()) == list(ref_att.state_dict())
res = ref_att.load_state_dict(our_att.state_dict(), strict=True)        # ours -> the reference's
assert not res.missing_keys and not res.unexpected_keys
res = our_net.load_state_dict(ref_net.state_dict(), strict=True)        # the reference's -> ours, whole container
assert not res.missing_keys and not res.unexpected_keys
assert list(our_net.state_dict()) == list(ref_net.state_dict())
for k, v in ref_net.state_dict().items():
    assert torch.equal(our_net.state_dict()[k], v), k
assert our_att.input_state_dimension == ref_att.input_state_dimension == H
assert our_att.output_state_dimension == ref_att.output_state_dimension == H


def minibatch(model):   # a fresh one per call: the reference's forward appends to `adjacency_lists` in place
    mb = model.initialize_minibatch()
    for gr in graphs:
        model.extend_minibatch_with(model.tensorize(gr), mb)
    return model.finalize_minibatch(mb, "cpu")


with torch.no_grad():
    want = ref_net.eval()(**minibatch(ref_model)).output_node_representations
    got = our_net.eval()(**minibatch(our_model)).output_node_representations
err_eval = float((got - want).abs().max())
assert err_eval <= TOL, f"eval: {err_eval:.3e}"

# The reference's window generator leaves autograd switched off for the attention (selfatt_cases.differentiable_reference):
# as shipped, its head transform gets no gradient at all.  Ours differentiates the attention, so the gradients are
# compared with the reference's operator sequence under autograd.
ref_net.train()
ref_net.zero_grad()
ref_net(**minibatch(ref_model)).output_node_representations.sum().backward()
assert next(ref_att.parameters()).grad is None
differentiable_reference(ref_module)

outs = []
for net, model in ((ref_net, ref_model), (our_net, our_model)):
    net.train()
    net.zero_grad()
    o = net(**minibatch(model)).output_node_representations
    (o * torch.linspace(-1, 1, o.numel()).view_as(o)).sum().backward()
    outs.append((o.detach(), {k: p.grad.clone() for k, p in net.named_parameters()}))
err_train = float((outs[0][0] - outs[1][0]).abs().max())
assert err_train <= TOL, f"train forward: {err_train:.3e}"
assert set(outs[0][1]) == set(outs[1][1])
err_grad = 0.0
for k, gr in outs[0][1].items():
    err_grad = max(err_grad, float((gr - outs[1][1][k]).abs().max()) / max(1.0, float(gr.abs().max())))
assert err_grad <= TOL, f"parameter gradients: {err_grad:.3e}"
print(f"SELFATT_DROPIN_OK eval={err_eval:.1e} train={err_train:.1e} grad={err_grad:.1e}")
