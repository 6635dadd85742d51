#!/usr/bin/env python
"""Generate tests/golden/embedder_*.npz from the REAL reference's TokenUnitEmbedder / SubtokenUnitEmbedder
(ptgnn/neuralmodels/embeddings/strelementrepresentationmodel.py:16-89), imported unmodified and executed on CPU in fp32
with the shims of make_golden.py (oracle/shims.py) and stand-ins for what the module imports at its top and only
StrElementRepresentationModel touches: `dpu_utils.codeutils.split_identifier_into_parts` and
`dpu_utils.mlutils.{Vocabulary, BpeVocabulary, CharTensorizer}`.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_embedder.py

Cases and inputs: tests/embedder_cases.py (dropout 0 everywhere).  Every fixture holds the arguments of `forward`
(`token_idxs`, `lengths`), `coef`, the module's initial state_dict under its seed (`state.<reference key>`), the output
`out` and the gradients of embedder_cases.loss_of with respect to every parameter (`grad.<reference key>`); `spec` is the
JSON of the case.
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


def install_embedder_shims():
    codeutils = types.ModuleType("dpu_utils.codeutils")
    codeutils.split_identifier_into_parts = lambda identifier: [identifier]
    mlutils = types.ModuleType("dpu_utils.mlutils")
    for name in ("Vocabulary", "BpeVocabulary", "CharTensorizer"):
        setattr(mlutils, name, type(name, (), {}))
    for name, mod in (("dpu_utils.codeutils", codeutils), ("dpu_utils.mlutils", mlutils)):
        sys.modules[name] = mod
        setattr(sys.modules["dpu_utils"], name.rsplit(".", 1)[1], mod)


install_embedder_shims()

from ptgnn.neuralmodels.embeddings import strelementrepresentationmodel as ref  # noqa: E402

from embedder_cases import CASES, build, loss_of, make_inputs  # noqa: E402


def main():
    for name, spec in CASES:
        args, coef = make_inputs(spec, torch.Generator().manual_seed(9100 + spec["seed"]))
        torch.manual_seed(spec["seed"])
        module = build(spec, ref)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        out = module(*args)
        loss = loss_of(out, args, coef)
        loss.backward()
        grads = {"grad." + k: p.grad for k, p in module.named_parameters()}
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
        arrays = dict(zip(("token_idxs", "lengths"), args))
        G.save(name, spec=np.asarray(json.dumps(spec)), coef=coef, out=out.detach(), **arrays, **state, **grads)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
