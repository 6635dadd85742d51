#!/usr/bin/env python
"""Generate tests/golden/attnpool_*.npz from the REAL reference's SelfAttentionVarSizedElementReduce and
MultiheadSelfAttentionVarSizedElementReduce (reduceops/varsizedsummary.py:84-178), imported unmodified and executed on
CPU in fp32 with the shims of make_golden.py (oracle/shims.py: torch_scatter restated, dpu_utils stubbed).

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_attnpool.py

Module specs: tests/attnpool_cases.py.  Every fixture holds an UNSORTED element -> sample map over NUM_SAMPLES samples
(SIZES: a 150-element sample, a 1-element one, an empty one in the middle and one past the largest index), x, the module's
initial state_dict under its seed (`state.<reference key>`), the output y and, for the loss sum(y * gout), the gradients
of x (`grad.x`) and of every parameter (`grad.<reference key>`); `spec` is the JSON of the case.
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

from ptgnn.neuralmodels.reduceops import varsizedsummary as ref  # noqa: E402

from attnpool_cases import CASES, NUM_SAMPLES, SIZES, build  # noqa: E402


def main():
    gen = torch.Generator().manual_seed(4242)
    for name, spec in CASES:
        idx = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
        idx = idx[torch.randperm(idx.shape[0], generator=gen)]
        x = torch.randn(idx.shape[0], spec["D"], generator=gen) * 1.5
        gout = torch.randn(NUM_SAMPLES, spec["out"], generator=gen)
        torch.manual_seed(spec["seed"])
        module = build(spec, ref)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        xr = x.clone().requires_grad_(True)
        y = module(ref.ElementsToSummaryRepresentationInput(xr, idx, NUM_SAMPLES))
        (y * gout).sum().backward()
        grads = {"grad.x": xr.grad}
        grads.update({"grad." + k: p.grad for k, p in module.named_parameters()})
        G.save(name, x=x, index=idx, num_samples=np.asarray(NUM_SAMPLES), y=y.detach(), gout=gout,
               spec=np.asarray(json.dumps(spec)), **state, **grads)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
