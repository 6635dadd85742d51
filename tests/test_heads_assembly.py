"""The Typilus, VarMisuse and PPI models assembled from ptgnn_amd classes only -- node embedder, message-passing layers,
container and task head, as the INTEGRATION snippets build them -- run one training step and report their metrics, on CPU
tensors and (marked gpu) on the MI355X."""
import math

import pytest
import torch
from torch import nn

import ptgnn_amd
from ptgnn_amd.embeddings import LinearFeatureEmbedder, SubtokenUnitEmbedder
from ptgnn_amd.gnn import GraphNeuralNetwork
from ptgnn_amd.layers import GatedMessagePassingLayer, MlpMessagePassingLayer

N, E, TYPES, D = 30, 90, 2, 16


def graph(gen, device, references, graphs):
    adj = [(torch.randint(0, N, (E,), generator=gen).to(device), torch.randint(0, N, (E,), generator=gen).to(device))
           for _ in range(TYPES)]
    return dict(adjacency_lists=adj, edge_feature_data=[], node_to_graph_idx=torch.arange(N).to(device) * graphs // N,
                reference_node_ids={k: v.to(device) for k, v in references.items()},
                reference_node_graph_idx={k: (v.to(device) if torch.is_tensor(v) else v) for k, v in references.items()},
                num_graphs=graphs)


def subtokens(gen, device):
    return dict(token_idxs=torch.randint(0, 50, (N, 4), generator=gen).to(device),
                lengths=torch.randint(1, 5, (N,), generator=gen).to(device))


def ggnn(embedder):
    layers = [GatedMessagePassingLayer(D, D, 2 * TYPES + 1, "max", dropout_rate=0.0) for _ in range(2)]
    return GraphNeuralNetwork(layers, embedder, introduce_backwards_edges=True, add_self_edges=True)


def typilus(gen, device):
    head = ptgnn_amd.Graph2ClassModule(ggnn(SubtokenUnitEmbedder(50, D, 0.0, "max")), 7)
    supernodes = torch.tensor([3, 11, 3, 29])
    data = graph(gen, device, {"supernodes": supernodes}, 3)
    data["reference_node_graph_idx"] = {"supernodes": torch.tensor([0, 1, 0, 2]).to(device)}
    return head, (dict(data, node_data=subtokens(gen, device)), torch.tensor([0, 6, 2, 5]).to(device), None)


def varmisuse(gen, device):
    head = ptgnn_amd.VarMisuseGraphModel(ggnn(SubtokenUnitEmbedder(50, D, 0.0, "mean")))
    data = graph(gen, device, {"candidate_nodes": torch.tensor([1, 2, 3, 14, 15]), "slot_node_idx": torch.tensor([0, 13])}, 2)
    data["reference_node_graph_idx"] = {"candidate_nodes": torch.tensor([0, 0, 0, 1, 1]).to(device)}
    return head, (dict(data, node_data=subtokens(gen, device)), torch.tensor([2, 3]).to(device))


def ppi(gen, device):
    layers = [MlpMessagePassingLayer(D, D, D, 2 * TYPES + 1, "sum", dropout_rate=0.0)]
    gnn = GraphNeuralNetwork(layers, LinearFeatureEmbedder(50, D, nn.Tanh()), introduce_backwards_edges=True,
                             add_self_edges=True)
    head = ptgnn_amd.PPIClassification(gnn, 11)
    data = graph(gen, device, {}, 1)
    features = torch.randn(N, 50, generator=gen).to(device)
    return head, (dict(data, node_data=dict(features=features)), (torch.rand(N, 11, generator=gen) < 0.3).to(device))


def step(make, device):
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    head, args = make(gen, device)
    head = head.to(device).train()
    loss = head(*args)
    loss.backward()
    assert loss.dtype == torch.float32 and math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters())
    metrics = head.report_metrics()
    assert all(math.isfinite(float(v)) for v in metrics.values())
    return float(loss.detach()), metrics


@pytest.mark.parametrize("make", [typilus, varmisuse, ppi], ids=["typilus", "varmisuse", "ppi"])
def test_models_assemble_from_ptgnn_amd_classes_on_cpu(make):
    loss, metrics = step(make, torch.device("cpu"))
    assert ("Accuracy" in metrics) != ("f1_score" in metrics)
    assert metrics["num_graphs"] >= 1                               # the container's metrics ride along


@pytest.mark.gpu
@pytest.mark.parametrize("make", [typilus, varmisuse, ppi], ids=["typilus", "varmisuse", "ppi"])
def test_models_assemble_from_ptgnn_amd_classes_on_the_gpu(make):
    loss, metrics = step(make, torch.device("cuda"))
    want, want_metrics = step(make, torch.device("cpu"))             # the same seed: the same parameters and inputs
    assert abs(loss - want) <= 2e-5 * max(1.0, abs(want))
    assert metrics.get("Accuracy") == want_metrics.get("Accuracy")
