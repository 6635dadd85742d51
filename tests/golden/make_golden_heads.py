#!/usr/bin/env python
"""Generate tests/golden/heads_*.npz from the REAL reference's task heads and feature embedder, imported unmodified and
executed on CPU in fp32 with the shims of make_golden.py (oracle/shims.py: torch_scatter restated, dpu_utils stubbed):

    Graph2ClassModule      ptgnn/implementations/typilus/graph2class.py:63-102
    VarMisuseGraphModel    ptgnn/implementations/varmisuse/varmisuse.py:41-91
    PPIClassification      ptgnn/implementations/ppi/ppi.py:13-62
    LinearFeatureEmbedder  ptgnn/neuralmodels/embeddings/linearmapembedding.py:13-29

and one more: three Generics of the reference answer the class itself when subscripted (see below).  The heads run around
the stub GNN of tests/head_cases.py (an nn.Module with `output_node_state_dim` that returns the reference's GnnOutput
holding the given node states, which require grad).

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_heads.py

Cases and inputs: tests/head_cases.py.  Every head fixture holds the inputs of two minibatches, the module's initial
state_dict under its seed (`state.<reference key>`), the loss of the first minibatch, the gradients of that loss with
respect to the node states (`grad.node_states`) and every parameter (`grad.<reference key>`), the metrics after the first
call (`metrics1.<name>`) and after the second (`metrics2.<name>`, `second.loss`), Graph2Class's `predict()` outputs
(`predict.probs`, `predict.classes`, `predict.graph_idx`) and `spec`, the JSON of the case.  The generator refuses a case
whose inputs miss the input conditions of tests/head_cases.py.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)
from make_golden_decoder import PART_BYTES, save_parts  # noqa: E402  (also installs dpu_utils.mlutils)

from ptgnn.neuralmodels.gnn import graphneuralnetwork, structs  # noqa: E402

# ppi.py:66, :73 and varmisuse.py:104 annotate with `TensorizedGraphData[np.ndarray]`, `GraphNeuralNetworkModel[np.ndarray,
# np.ndarray]` and `GraphData[Tuple[str, bool]]` -- fewer parameters than the Generics have, which this Python's typing
# refuses at import.  The subscripts are annotations only: let them answer the class itself.
for _generic in (structs.TensorizedGraphData, structs.GraphData, graphneuralnetwork.GraphNeuralNetworkModel):
    _generic.__class_getitem__ = classmethod(lambda cls, params: cls)

# varmisuse.py:5 imports a tokeniser only VarMisuseModel's tensorisation uses: an identity stand-in
_codeutils = types.ModuleType("dpu_utils.codeutils")
_codeutils.split_identifier_into_parts = lambda identifier: [identifier]
sys.modules["dpu_utils.codeutils"] = _codeutils
sys.modules["dpu_utils"].codeutils = _codeutils

from ptgnn.implementations.ppi.ppi import PPIClassification  # noqa: E402
from ptgnn.implementations.typilus.graph2class import Graph2ClassModule  # noqa: E402
from ptgnn.implementations.varmisuse.varmisuse import VarMisuseGraphModel  # noqa: E402
from ptgnn.neuralmodels.embeddings.linearmapembedding import LinearFeatureEmbedder  # noqa: E402
from ptgnn.neuralmodels.gnn.structs import GnnOutput  # noqa: E402

from head_cases import ALL_HEAD_CASES, LFE_CASES, build, build_lfe, call_args, conditions_hold, make_inputs  # noqa: E402

REF = types.SimpleNamespace(Graph2ClassModule=Graph2ClassModule, VarMisuseGraphModel=VarMisuseGraphModel,
                            PPIClassification=PPIClassification, LinearFeatureEmbedder=LinearFeatureEmbedder)


def heads():
    for kind, name, spec in ALL_HEAD_CASES:
        inputs = make_inputs(kind, spec, torch.Generator().manual_seed(9000 + spec["seed"]))
        torch.manual_seed(spec["seed"])
        module = build(kind, spec, REF, GnnOutput)
        arrays = dict(inputs, spec=np.asarray(json.dumps(spec)))
        arrays.update({"state." + k: v.detach().clone() for k, v in module.state_dict().items()})
        if kind == "g2c":
            with torch.no_grad():
                probs, classes, graph_idx = module.predict(call_args(kind, inputs)[0])
            arrays.update({"predict.probs": probs, "predict.classes": classes, "predict.graph_idx": graph_idx})
        module.reset_metrics()
        states = inputs["node_states"].clone().requires_grad_(True)
        loss = module(*call_args(kind, inputs, states=states))
        loss.backward()
        arrays["loss"] = loss.detach()
        arrays["grad.node_states"] = states.grad
        arrays.update({"grad." + k: p.grad.clone() for k, p in module.named_parameters()})
        arrays.update({"metrics1." + k: np.asarray(float(v)) for k, v in module.report_metrics().items()})
        with torch.no_grad():
            arrays["second.loss"] = module(*call_args(kind, inputs, second=True))
        arrays.update({"metrics2." + k: np.asarray(float(v)) for k, v in module.report_metrics().items()})
        assert all(bool(torch.isfinite(v).all()) for k, v in arrays.items()
                   if isinstance(v, torch.Tensor) and v.is_floating_point()), name
        check = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
        assert conditions_hold(kind, check), f"{name}: the inputs of seed {spec['seed']} miss the input conditions"
        assert sum(v.nbytes for v in check.values()) < PART_BYTES, name
        save_parts(name, arrays)


def embedders():
    for name, spec in LFE_CASES:
        gen = torch.Generator().manual_seed(9000 + spec["seed"])
        features = torch.randn(spec["N"], spec["F"], generator=gen)
        cotangent = torch.randn(spec["N"], spec["D"], generator=gen)
        torch.manual_seed(spec["seed"])
        module = build_lfe(spec, REF)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        x = features.clone().requires_grad_(True)
        out = module(x)
        (out * cotangent).sum().backward()
        grads = {"grad." + k: p.grad for k, p in module.named_parameters()}
        save_parts(name, dict(features=features, cotangent=cotangent, out=out.detach(), spec=np.asarray(json.dumps(spec)),
                              **{"grad.features": x.grad}, **state, **grads))


if __name__ == "__main__":
    torch.set_num_threads(1)
    heads()
    embedders()
