"""Cases of the char-CNN embedder fixtures: tests/golden/make_golden_charcnn.py builds the module from the reference's
classes (strelementrepresentationmodel.py:92-142), tests/test_char_embedder_cpu.py and tests/test_gpu_char_embedder.py
from ptgnn_amd.embeddings; plus the inputs of a case and a plain-torch restatement of the forward (unfold + matmul, no
conv1d) in any dtype -- the float64 yardstick of the GPU tests.

A case is C (characters), L (max_num_chars), the filter counts F1 / F2, the window sizes k = (k1, k2, k3), D (embedding
size) and B samples.  `small` is the standard windowed route, `windows_243` has unequal windows, `min_length` has
L = k1 + k2 + k3 - 2 (a single output position), `padded` holds 1-4 live characters followed by id 0 the way CharTensorizer
pads short strings (repeated windows, tied maxima), `odd` has widths that are not multiples of 4 (the composed route).
The loss behind the gradients is sum(out * coef)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [
    ("charcnn_small", dict(C=40, L=15, F1=64, F2=32, k=[3, 3, 3], D=64, B=9, padded=False, seed=51)),
    ("charcnn_windows_243", dict(C=12, L=11, F1=8, F2=12, k=[2, 4, 3], D=8, B=7, padded=False, seed=52)),
    ("charcnn_min_length", dict(C=12, L=7, F1=8, F2=8, k=[3, 3, 3], D=8, B=5, padded=False, seed=53)),
    ("charcnn_padded", dict(C=20, L=15, F1=16, F2=8, k=[3, 3, 3], D=16, B=8, padded=True, seed=54)),
    ("charcnn_odd", dict(C=11, L=9, F1=6, F2=12, k=[3, 3, 3], D=10, B=6, padded=False, seed=55)),
]

PARAMS = ["_CharUnitEmbedder__conv_l1.weight", "_CharUnitEmbedder__conv_l1.bias", "_CharUnitEmbedder__conv_l2.weight",
          "_CharUnitEmbedder__conv_l2.bias", "_CharUnitEmbedder__conv_l3.weight"]


def build(spec, ns, dropout_rate=0.0):
    """The embedder of `spec` from the namespace `ns` (a module holding CnnConfig / CharUnitEmbedder)."""
    k1, k2, k3 = spec["k"]
    return ns.CharUnitEmbedder(spec["C"], spec["D"], ns.CnnConfig(spec["F1"], k1, spec["F2"], k2, k3), dropout_rate)


def make_chars(B, L, C, gen, padded=False):
    chars = torch.randint(1 if padded else 0, C, (B, L), generator=gen)
    if padded:
        for b in range(B):
            chars[b, 1 + b % 4:] = 0          # 1-4 live characters, then the padding id
    return chars


def make_inputs(spec, gen):
    """(chars [B, L], coef [B, D]) for `spec`, drawn from `gen` (CPU tensors)."""
    chars = make_chars(spec["B"], spec["L"], spec["C"], gen, spec["padded"])
    return chars, torch.randn(spec["B"], spec["D"], generator=gen)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def _conv(x, weight, bias):
    """nn.Conv1d over the channel-last x [B, P, C_in] as unfold + matmul: [B, P - k + 1, F]."""
    n_out, _, k = weight.shape
    windows = x.unfold(1, k, 1)                                            # [B, P', C_in, k]
    y = torch.matmul(windows.reshape(x.shape[0], windows.shape[1], -1), weight.reshape(n_out, -1).t())
    return y if bias is None else y + bias


def ref_layers(chars, params, dtype):
    """(a1, a2, l3, out) of strelementrepresentationmodel.py:133-142 restated channel-last in `dtype` on the device of
    `chars`; `params` = the five tensors in PARAMS order."""
    w1, b1, w2, b2, w3 = (p.to(dtype) for p in params)
    x = torch.eye(w1.shape[1], dtype=dtype, device=chars.device)[chars]   # [B, L, C]
    a1 = torch.relu(_conv(x, w1, b1))
    a2 = torch.relu(_conv(a1, w2, b2))
    l3 = _conv(a2, w3, None)
    return a1, a2, l3, l3.max(dim=1)[0]


def ref_forward(chars, params, dtype):
    return ref_layers(chars, params, dtype)[3]


def reference(chars, params, coef, dtype):
    """(out, [d param ...]) of the restatement in `dtype` on the CPU for the loss sum(out * coef)."""
    leaves = [p.detach().cpu().to(dtype).requires_grad_(True) for p in params]
    out = ref_forward(chars.cpu(), leaves, dtype)
    (out * coef.cpu().to(dtype)).sum().backward()
    return out.detach(), [p.grad for p in leaves]
