"""Opt-in 16-bit matrix-core inputs for the GGNN layer's dense blocks.

The default is `torch.float32`: every dense block runs the exact-fp32 MFMA kernels, bit for bit as without this module.
With `torch.bfloat16` / `torch.float16` the INFERENCE routes of `GatedMessagePassingLayer` round the operands of the
table-form message Linear and of the GRU cell's gate GEMMs to that type (round to nearest even, like `tensor.to(dtype)`)
and multiply them on the 16-bit matrix cores (csrc/half_gemm.hip); accumulation, bias, gate math, the aggregation and
the stored states stay fp32.  That is what an `enable_amp` user of the reference trainer gets from autocast
(trainer.py:205,221; the reference up-casts only at the scatter, abstractmessagepassing.py:43-50).

    ptgnn_amd.set_matrix_inputs("autocast")       # next to enable_amp: follow torch.autocast on GPU tensors
    with ptgnn_amd.matrix_inputs(torch.bfloat16): # or explicitly, for a block
        out = model(batch)

What stays fp32 under the setting: every training route (anything that needs a gradient), `forward_sharded`, the
grouped per-edge GEMM of the edge form, every other layer and the decoder.  Shapes the 16-bit kernels do not take
(widths that are not multiples of 32) run the fp32 kernels, silently.  CPU tensors (ptgnn_amd/torch_route.py) round the
same operands with torch, so a checkpoint behaves alike on both devices; "autocast" never touches CPU tensors.

The setting is process-wide (like `ops.set_gemm_mode`); the layers read it, `ptgnn_amd.ops` never does -- its
`inputs=` keyword is explicit, because inside an autograd `Function.forward` grad mode is off and an op could not tell
inference from training.
"""
import contextlib

import torch

from ptgnn_amd._lib import PtgnnAmdError

HALF_DTYPES = (torch.bfloat16, torch.float16)
_CHOICES = (torch.float32,) + HALF_DTYPES + ("autocast",)

_setting = torch.float32


def _checked(v):
    if not isinstance(v, (torch.dtype, str)) or v not in _CHOICES:
        raise PtgnnAmdError(f"matrix inputs must be torch.float32, torch.bfloat16, torch.float16 or 'autocast' (got {v!r})")
    return v


def set_matrix_inputs(v):
    """Set the operand type of the GGNN inference GEMMs; returns the previous setting."""
    global _setting
    prev, _setting = _setting, _checked(v)
    return prev


def get_matrix_inputs():
    return _setting


@contextlib.contextmanager
def matrix_inputs(v):
    prev = set_matrix_inputs(v)
    try:
        yield
    finally:
        set_matrix_inputs(prev)


def resolve(tensor: torch.Tensor) -> torch.dtype:
    """The dtype the setting means for a layer call on `tensor`: "autocast" is the CUDA autocast dtype for a GPU tensor
    while autocast is enabled (when that is a 16-bit type), else float32."""
    v = _setting
    if v == "autocast":
        if tensor.is_cuda and torch.is_autocast_enabled("cuda"):
            dt = torch.get_autocast_dtype("cuda")
            return dt if dt in HALF_DTYPES else torch.float32
        return torch.float32
    return v
