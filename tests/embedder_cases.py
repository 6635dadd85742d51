"""Cases of the node-embedder fixtures: tests/golden/make_golden_embedder.py builds the modules from the reference's
classes (strelementrepresentationmodel.py:16-89), tests/test_embedder_cpu.py and tests/test_gpu_embedder.py from
ptgnn_amd.embeddings; plus the inputs of a case and a plain-torch restatement of the subtoken pool in any dtype (the
float64 yardstick of the GPU tests).

A case is `kind` ("token" or a subtoken combination), V (vocabulary), D (embedding), S (max_num_subtokens), B bags and
whether the dense output layer exists.  Every subtoken case repeats one id in two live slots of bag 0, has lengths 1 and
S, and a length of S + 2 (the reference masks nothing there and, for mean, divides by the given length); `zero` adds a bag
without subtokens (output 0, or -inf for max -- not in front of the dense layer, where the reference yields NaN).  The
loss behind the gradients is sum(out * coef) over the bags with a subtoken."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [
    ("embedder_sum_d64", dict(kind="sum", V=200, D=64, S=5, B=40, dense=True, zero=True, seed=31)),
    ("embedder_sum_d128", dict(kind="sum", V=90, D=128, S=5, B=41, dense=True, zero=True, seed=32)),
    ("embedder_mean_d64", dict(kind="mean", V=150, D=64, S=5, B=39, dense=True, zero=True, seed=33)),
    ("embedder_mean_d128", dict(kind="mean", V=50, D=128, S=5, B=40, dense=True, zero=True, seed=34)),
    ("embedder_max_d64", dict(kind="max", V=200, D=64, S=5, B=40, dense=True, zero=False, seed=35)),
    ("embedder_max_d128", dict(kind="max", V=70, D=128, S=5, B=43, dense=True, zero=False, seed=36)),
    ("embedder_max_pool", dict(kind="max", V=120, D=64, S=5, B=40, dense=False, zero=True, seed=37)),
    ("embedder_token", dict(kind="token", V=100, D=64, S=1, B=40, dense=False, zero=False, seed=38)),
]


def build(spec, ns, dropout_rate=0.0):
    """The embedder of `spec` from the namespace `ns` (a module holding TokenUnitEmbedder / SubtokenUnitEmbedder)."""
    if spec["kind"] == "token":
        return ns.TokenUnitEmbedder(spec["V"], spec["D"], dropout_rate)
    return ns.SubtokenUnitEmbedder(spec["V"], spec["D"], dropout_rate, spec["kind"], use_dense_output=spec["dense"])


def make_inputs(spec, gen):
    """(positional arguments of the module's forward, coef [B, D]) for `spec`, drawn from `gen` (CPU tensors)."""
    B, S, V, D = spec["B"], spec["S"], spec["V"], spec["D"]
    coef = torch.randn(B, D, generator=gen)
    if spec["kind"] == "token":
        return (torch.randint(0, V, (B,), generator=gen),), coef
    ids = torch.randint(0, V - 3, (B, S), generator=gen)         # the last three vocabulary rows are never referenced
    lengths = torch.randint(1, S + 1, (B,), generator=gen)
    ids[0, 1] = ids[0, 0]                                        # one id in two live slots of a bag
    lengths[0], lengths[1], lengths[4], lengths[5] = 2, 1, S, S + 2
    if spec["zero"]:
        lengths[2] = 0
    return (ids, lengths), coef


def loss_of(out, args, coef):
    """sum(out * coef) over the bags that have a subtoken (every row of the token embedder)."""
    keep = args[1] > 0 if len(args) == 2 else torch.ones(out.shape[0], dtype=torch.bool, device=out.device)
    return (out[keep] * coef[keep]).sum()


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def args_of(fx, to=lambda t: t):
    keys = ("token_idxs", "lengths") if "lengths" in fx else ("token_idxs",)
    return tuple(to(torch.from_numpy(fx[k])) for k in keys)


def ref_pool(table, ids, lengths, kind):
    """strelementrepresentationmodel.py:67-82 restated without the in-place fill, in the dtype / on the device of `table`."""
    S = ids.shape[1]
    live = (torch.arange(S, device=ids.device).unsqueeze(0) < lengths.unsqueeze(-1)).unsqueeze(-1)
    embedded = table[ids]
    if kind == "max":
        return embedded.masked_fill(~live, float("-inf")).max(dim=-2)[0]
    pooled = (embedded * live.to(table.dtype)).sum(dim=-2)
    if kind == "mean":
        # the divisor is rounded in float32, as the reference and the kernel round it
        pooled = pooled / (lengths.unsqueeze(-1).float() + 1e-10).to(table.dtype)
    return pooled
