#!/usr/bin/env python
"""Generate tests/golden/graph2seq_*.npz from the REAL reference's Graph2SeqModule
(ptgnn/implementations/graph2seq/graph2seq.py:36-81), imported unmodified and executed on CPU in fp32 with the shims of
make_golden.py and make_golden_decoder.py, around the stub GNN of tests/graph2seq_cases.py (an nn.Module that returns the
reference's GnnOutput holding the given node states), the reference's MultiheadSelfAttentionVarSizedElementReduce with
SimpleVarSizedElementReduce("max") and the reference's GruCopyingDecoder.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_graph2seq.py

Cases and inputs: tests/graph2seq_cases.py (dropout 0).  Every fixture holds the inputs of two minibatches, the module's
initial state_dict under its seed (`state.<reference key>`), the loss of the first minibatch, the gradients of that loss
with respect to both node-state tensors (`grad.input_states`, `grad.output_states`) and every parameter
(`grad.<reference key>`), the metrics after the first call (`metrics1.loss`) and after the second (`metrics2.loss`,
`second.loss`) and `spec`, the JSON of the case.  A fixture past PART_BYTES continues in `name.pK.npz`, and an array too
large for one file is stored as row blocks (graph2seq_cases.pieces / load).  The generator refuses a case whose inputs miss the input conditions of tests/graph2seq_cases.py.
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

import make_golden as G  # noqa: E402,F401  (installs the shims, puts the reference on sys.path)
import make_golden_decoder  # noqa: E402  (also installs dpu_utils.mlutils and scatter_logsumexp)
from make_golden_decoder import save_parts  # noqa: E402

make_golden_decoder.PART_BYTES = 600_000       # uncompressed bytes per part: every file stays under 700 000 on disk

from ptgnn.neuralmodels.gnn import graphneuralnetwork, structs  # noqa: E402

# graph2seq.py subscripts Generics of the reference in annotations with fewer parameters than they have, which this
# Python's typing refuses at import: let the subscripts answer the class itself (as make_golden_heads.py does)
for _generic in (structs.TensorizedGraphData, structs.GraphData, graphneuralnetwork.GraphNeuralNetworkModel):
    _generic.__class_getitem__ = classmethod(lambda cls, params: cls)

from ptgnn.implementations.graph2seq.graph2seq import Graph2SeqModule  # noqa: E402
from ptgnn.neuralmodels.gnn.structs import GnnOutput  # noqa: E402
from ptgnn.neuralmodels.reduceops import (  # noqa: E402
    MultiheadSelfAttentionVarSizedElementReduce, SimpleVarSizedElementReduce)
from ptgnn.neuralmodels.sequence.grucopydecoder import GruCopyingDecoder  # noqa: E402

from graph2seq_cases import CASES, build, call_args, conditions_hold, make_inputs, pieces  # noqa: E402

REF = types.SimpleNamespace(Graph2SeqModule=Graph2SeqModule, GruCopyingDecoder=GruCopyingDecoder,
                            MultiheadSelfAttentionVarSizedElementReduce=MultiheadSelfAttentionVarSizedElementReduce,
                            SimpleVarSizedElementReduce=SimpleVarSizedElementReduce)


def main():
    for name, spec in CASES:
        inputs = make_inputs(spec, torch.Generator().manual_seed(9000 + spec["seed"]))
        assert conditions_hold(spec, inputs), f"{name}: the inputs of seed {spec['seed']} miss the input conditions"
        torch.manual_seed(spec["seed"])
        module = build(spec, REF, GnnOutput)
        arrays = dict(inputs, spec=np.asarray(json.dumps(spec)))
        arrays.update({"state." + k: v.detach().clone() for k, v in module.state_dict().items()})
        module.reset_metrics()
        states = tuple(inputs[k].clone().requires_grad_(True) for k in ("input_states", "output_states"))
        loss = module(**call_args(spec, inputs, states=states))
        loss.backward()
        arrays["loss"] = loss.detach()
        arrays["grad.input_states"], arrays["grad.output_states"] = states[0].grad, states[1].grad
        arrays.update({"grad." + k: p.grad.clone() for k, p in module.named_parameters()})
        arrays.update({"metrics1." + k: np.asarray(float(v)) for k, v in module.report_metrics().items()})
        with torch.no_grad():
            arrays["second.loss"] = module(**call_args(spec, inputs, second=True))
        arrays.update({"metrics2." + k: np.asarray(float(v)) for k, v in module.report_metrics().items()})
        assert all(bool(torch.isfinite(v).all()) for v in arrays.values()
                   if isinstance(v, torch.Tensor) and v.is_floating_point()), name
        arrays = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
        save_parts(name, dict(piece for k, v in arrays.items() for piece in pieces(k, v)))


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
