#!/usr/bin/env python
"""Generate tests/golden/graphnorm_*.npz from the REAL reference's GraphNorm
(gnn/messagepassing/graphnorm.py:9-54), imported unmodified and executed on CPU with the shims of make_golden.py
(oracle/shims.py: torch_scatter restated, dpu_utils stubbed) -- once in fp32 and once as the same module under
`.double()`.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_graphnorm.py

Case specs: tests/graphnorm_cases.py.  Every fixture holds an UNSORTED node -> graph map over NUM_GRAPHS graphs (COUNTS:
a 70-node graph, a 1-node one, an empty one in the middle, a 2-node one and an empty one behind them), x, the layer's
state (`state.gamma/alpha/bias`), gout, the output y and, for the loss sum(y * gout), the gradients of x (`grad.x`) and of
every parameter (`grad.<name>`) in fp32, the same in float64 (`y64`, `grad64.*`); `spec` is the JSON of the case.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from ptgnn.neuralmodels.gnn.messagepassing import graphnorm as ref  # noqa: E402

from graphnorm_cases import CASES, EXTRA_INDEX, SIZES, build  # noqa: E402


def run(module, x, idx, gout):
    xr = x.clone().requires_grad_(True)
    y = module(xr, [], idx, {}, {}, [])
    (y * gout).sum().backward()
    grads = {"x": xr.grad}
    grads.update({k: p.grad for k, p in module.named_parameters()})
    return y.detach(), grads


def main():
    for name, spec in CASES:
        gen = torch.Generator().manual_seed(4300 + spec["seed"])
        D = spec["D"]
        idx = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
        idx = torch.cat([idx, torch.tensor([EXTRA_INDEX])])
        idx = idx[torch.randperm(idx.shape[0], generator=gen)]
        x = torch.randn(idx.shape[0], D, generator=gen) * 1.5
        gout = torch.randn(idx.shape[0], D, generator=gen)
        module = build(spec, ref)
        if spec["random_params"]:
            with torch.no_grad():
                module.gamma.copy_(0.5 + torch.rand(1, D, generator=gen))
                module.alpha.copy_(0.5 + torch.rand(1, D, generator=gen))
                module.bias.copy_(torch.randn(1, D, generator=gen))
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        y, grads = run(module, x, idx, gout)
        y64, grads64 = run(copy.deepcopy(module).double(), x.double(), idx, gout.double())
        G.save(name, x=x, index=idx, gout=gout, y=y, y64=y64, spec=np.asarray(json.dumps(spec)), **state,
               **{"grad." + k: v for k, v in grads.items()}, **{"grad64." + k: v for k, v in grads64.items()})


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
