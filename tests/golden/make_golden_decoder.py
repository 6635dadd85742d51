#!/usr/bin/env python
"""Generate tests/golden/decoder_*.npz from the REAL reference's GruCopyingDecoder
(ptgnn/neuralmodels/sequence/grucopydecoder.py:29-212), imported unmodified and executed on CPU in fp32 with the shims of
make_golden.py (oracle/shims.py: torch_scatter restated, dpu_utils stubbed) and two additions the decoder's module needs
before it imports:
  * `dpu_utils.mlutils.Vocabulary` (only GruCopyingDecoderModel touches it): an empty stand-in class;
  * `scatter_logsumexp` of torch_scatter 2.0.x, restated here from its published algorithm (composite/logsumexp.py): the
    per-segment maximum over a -inf initialised buffer, `log(sum exp(src - max) + eps) + max`.

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_decoder.py

Cases and inputs: tests/decoder_cases.py (dropout 0 everywhere).  Every fixture holds the keyword arguments of `forward`,
the module's initial state_dict under its seed (`state.<reference key>`), the loss, the three outputs of
`_compute_logprobs` (`copy_logprobs`, `target_logprobs`, `gru_state`) and the gradients of the loss with respect to
input_memories, initial_states (`grad.input_memories`, `grad.initial_states`) and every parameter
(`grad.<reference key>`); `spec` is the JSON of the case.  A fixture past PART_BYTES continues in `name.pK.npz`
(decoder_cases.load reads the parts back as one dict).
"""
import glob
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


def scatter_logsumexp(src, index, dim=-1, out=None, dim_size=None, eps=1e-12):
    """torch_scatter.composite.scatter_logsumexp, 2.0.x, for a 1-D index along dim 0 of a 1-D / 2-D src."""
    assert out is None and index.dim() == 1 and dim % src.dim() == 0
    n = int(index.max()) + 1 if dim_size is None else int(dim_size)
    idx = index if src.dim() == 1 else index.unsqueeze(1).expand_as(src)
    top = torch.full((n,) + tuple(src.shape[1:]), float("-inf"), dtype=src.dtype).scatter_reduce(
        0, idx, src.detach(), "amax", include_self=True)
    shift = top.gather(0, idx)
    rec = src - shift
    rec = rec.masked_fill(rec.isnan(), float("-inf"))
    total = torch.zeros_like(top).scatter_add(0, idx, rec.exp())
    return (total + eps).log() + top


def install_decoder_shims():
    mlutils = types.ModuleType("dpu_utils.mlutils")
    mlutils.Vocabulary = type("Vocabulary", (), {})
    sys.modules["dpu_utils.mlutils"] = mlutils
    sys.modules["dpu_utils"].mlutils = mlutils
    for name in ("torch_scatter", "torch_scatter.composite"):
        sys.modules[name].scatter_logsumexp = scatter_logsumexp


install_decoder_shims()

from ptgnn.neuralmodels.sequence import grucopydecoder as ref  # noqa: E402

from decoder_cases import CASES, build, make_inputs  # noqa: E402

PART_BYTES = 700_000


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
    for name, spec in CASES:
        inputs = make_inputs(spec, torch.Generator().manual_seed(9000 + spec["seed"]))
        torch.manual_seed(spec["seed"])
        module = build(spec, ref)
        state = {"state." + k: v.detach().clone() for k, v in module.state_dict().items()}
        memories = inputs["input_memories"].clone().requires_grad_(True)
        states = inputs["initial_states"].clone().requires_grad_(True)
        live = dict(inputs, input_memories=memories, initial_states=states)
        with torch.no_grad():
            copy_logprobs, target_logprobs, gru_state = module._compute_logprobs(
                states, memories, inputs["input_memories_origin_idx"], inputs["target_token_ids"][:, :-1])
        loss = module(**live)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(memories.grad).all())
        grads = {"grad.input_memories": memories.grad, "grad.initial_states": states.grad}
        grads.update({"grad." + k: p.grad for k, p in module.named_parameters()})
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        save_parts(name, dict(inputs, spec=np.asarray(json.dumps(spec)), loss=loss.detach(), copy_logprobs=copy_logprobs,
                              target_logprobs=target_logprobs, gru_state=gru_state, **state, **grads))


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
