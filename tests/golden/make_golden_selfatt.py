#!/usr/bin/env python
"""Generate tests/golden/selfatt_*.npz from the REAL reference's MultiHeadSelfAttentionMessagePassing
(gnn/messagepassing/selfattmessagepassing.py:9-136), imported unmodified and executed on CPU with the shims of
make_golden.py, in eval mode with dropout_rate = 0 -- once in fp32 and once as the same module under `.double()`.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_selfatt.py

Gradients.  The reference's window generator (selfattmessagepassing.py:59-75) yields from inside `with torch.no_grad()`,
and a suspended generator leaves the grad mode it set behind: the loop body of lines 105-115 -- the attention itself --
runs without autograd, so the unmodified class gives the head transform NO gradient and the input only the gradient of
the residual path.  The fixtures hold the gradients of the function the forward computes: the class text is untouched,
but the name `torch` of its module is bound to a stand-in whose `no_grad()` does nothing (`differentiable_reference`),
so torch's autograd runs through the reference's own einsum / softmax / einsum.  The forward values do not change.
ptgnn_amd's layer differentiates the attention (a documented difference from the reference's behaviour).

Case specs: tests/selfatt_cases.py.  Every fixture holds x, the node -> graph index (`index`; for the target case also
`ids`, a permutation of all nodes, and then `index` is reference_node_graph_idx), gout, the layer's state (`state.*`), the
output y and, for the loss sum(y * gout), the gradients of x (`grad.x`) and of every parameter (`grad.<name>`) in fp32,
the same in float64 (`y64`, `grad64.*`); `spec` is the JSON of the case.  A fixture that outgrows one committed file is
continued in `name.pK.npz` (selfatt_cases.load reads the parts back as one dict).
"""
import copy
import glob
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from ptgnn.neuralmodels.gnn.messagepassing import selfattmessagepassing as ref  # noqa: E402

from selfatt_cases import CASES, PART_BYTES, TARGET, build, differentiable_reference, sizes  # noqa: E402


def run(module, spec, x, idx, ids, gout):
    xr = x.clone().requires_grad_(True)
    if spec["target"]:    # the reference assigns into its input: hand it a copy that autograd may overwrite
        y = module(xr * 1.0, [], torch.zeros(x.shape[0], dtype=torch.int64), {TARGET: ids}, {TARGET: idx}, [])
    else:
        y = module(xr, [], idx, {}, {}, [])
    (y * gout).sum().backward()
    grads = {"x": xr.grad}
    grads.update({k: p.grad for k, p in module.named_parameters()})
    return y.detach(), grads


def save_parts(name, arrays):
    for old in glob.glob(os.path.join(G.OUT, name + "*.npz")):
        os.remove(old)
    arrays = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
    parts, used = [{}], 0
    for k, v in arrays.items():
        if used and used + v.nbytes > PART_BYTES:
            parts.append({})
            used = 0
        parts[-1][k] = v
        used += v.nbytes
    for i, part in enumerate(parts):
        G.save(name if i == 0 else f"{name}.p{i}", **part)


def main():
    probe = build(CASES[0][1], ref)
    probe(torch.randn(5, CASES[0][1]["D"]), [], torch.zeros(5, dtype=torch.int64), {}, {}, []).sum().backward()
    assert next(probe.parameters()).grad is None          # the unmodified class: no gradient reaches the head transform
    differentiable_reference(ref)
    for name, spec in CASES:
        gen = torch.Generator().manual_seed(4400 + spec["seed"])
        D = spec["D"]
        counts = sizes(spec["max"])
        idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
        if spec["unsorted"]:
            idx = idx[torch.randperm(idx.shape[0], generator=gen)]
        n = idx.shape[0]
        ids = torch.randperm(n, generator=gen) if spec["target"] else None
        x = torch.randn(n, D, generator=gen) * spec["scale"]
        gout = torch.randn(n, D, generator=gen)
        torch.manual_seed(4500 + spec["seed"])
        module = build(spec, ref).eval()
        with torch.no_grad():       # LayerNorm and the biases off their initial ones / zeros
            for k, p in module.named_parameters():
                if "layer_norm" in k:
                    p.copy_((0.5 + torch.rand(p.shape, generator=gen)) if k.endswith("weight")
                            else torch.randn(p.shape, generator=gen) * 0.5)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        y, grads = run(module, spec, x, idx, ids, gout)
        y64, grads64 = run(copy.deepcopy(module).double(), spec, x.double(), idx, ids, gout.double())
        arrays = dict(spec=np.asarray(json.dumps(spec)), index=idx, x=x, gout=gout, y=y, **state,
                      **{"grad." + k: v for k, v in grads.items()})
        if ids is not None:
            arrays["ids"] = ids
        arrays.update(y64=y64, **{"grad64." + k: v for k, v in grads64.items()})
        save_parts(name, arrays)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
