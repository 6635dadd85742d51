#!/usr/bin/env python
"""Generate tests/golden/charcnn_*.npz from the REAL reference's CharUnitEmbedder / CnnConfig
(ptgnn/neuralmodels/embeddings/strelementrepresentationmodel.py:92-142), imported unmodified and executed on CPU in fp32
with the shims of make_golden.py (oracle/shims.py) and the stand-ins of make_golden_embedder.py for what the module
imports at its top and only StrElementRepresentationModel touches.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_charcnn.py

Cases and inputs: tests/char_embedder_cases.py (dropout 0 everywhere).  Every fixture holds `chars`, `coef`, the module's
initial state_dict under its seed (`state.<reference key>`), the output `out` and the gradients of sum(out * coef) with
respect to every parameter (`grad.<reference key>`); `spec` is the JSON of the case.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)
import make_golden_embedder  # noqa: E402,F401  (installs the dpu_utils stand-ins)

from ptgnn.neuralmodels.embeddings import strelementrepresentationmodel as ref  # noqa: E402

from char_embedder_cases import CASES, build, make_inputs  # noqa: E402


def main():
    for name, spec in CASES:
        chars, coef = make_inputs(spec, torch.Generator().manual_seed(9200 + spec["seed"]))
        torch.manual_seed(spec["seed"])
        module = build(spec, ref)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        out = module(chars)
        loss = (out * coef).sum()
        loss.backward()
        grads = {"grad." + k: p.grad for k, p in module.named_parameters()}
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        G.save(name, spec=np.asarray(json.dumps(spec)), chars=chars, coef=coef, out=out.detach(), **state, **grads)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
