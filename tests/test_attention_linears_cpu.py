"""The `linears=` keyword of `ptgnn_amd.set_attention_training` and the shape check of the panel-form 16-bit Linear
(csrc/panel_linear16.hip), without a GPU."""
import pytest
import torch

import ptgnn_amd
from ptgnn_amd import ops, precision


def test_keyword_is_off_by_default_and_the_plain_switch_leaves_the_linears_fp32(monkeypatch):
    x = torch.zeros(2, 2)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))    # a GPU tensor, as the readers see one
    with ptgnn_amd.matrix_inputs(torch.bfloat16):
        assert precision.attention_linear_inputs(x) == torch.float32
        assert ptgnn_amd.set_attention_training(True) is False
        assert precision.attention_training_inputs(x) == torch.bfloat16
        assert precision.attention_linear_inputs(x) == torch.float32
        assert ptgnn_amd.set_attention_training(True, linears=True) is True
        assert ptgnn_amd.attention_linear_inputs(x) == torch.bfloat16
        assert ptgnn_amd.set_attention_training(False, linears=True) is True     # linears without the switch: off
        assert precision.attention_linear_inputs(x) == precision.attention_training_inputs(x) == torch.float32
    with ptgnn_amd.attention_training(linears=True):                             # a float32 dtype setting means fp32
        assert precision.attention_linear_inputs(x) == torch.float32


def test_context_manager_restores_both_values_and_cpu_tensors_resolve_to_float32(monkeypatch):
    x = torch.zeros(2, 2)
    with ptgnn_amd.matrix_inputs(torch.float16), ptgnn_amd.attention_training(linears=True):
        assert precision.attention_linear_inputs(x) == torch.float32             # a CPU tensor
        with ptgnn_amd.attention_training():                                     # the plain switch inside
            assert (precision._attention_training, precision._attention_linears) == (True, False)
        assert (precision._attention_training, precision._attention_linears) == (True, True)
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        assert precision.attention_linear_inputs(x) == torch.float16
    assert (precision._attention_training, precision._attention_linears) == (False, False)


@pytest.mark.parametrize("k, n_out, dt, ok", [
    (32, 32, torch.bfloat16, True), (256, 1024, torch.float16, True), (4096, 4096, torch.bfloat16, True),
    (96, 160, torch.float16, True), (48, 64, torch.bfloat16, False), (64, 80, torch.bfloat16, False),
    (4128, 64, torch.float16, False), (64, 4128, torch.float16, False), (0, 64, torch.bfloat16, False),
    (64, 64, torch.float32, False)])
def test_panel_linear16_supported_accepts_and_refuses_the_documented_shapes(k, n_out, dt, ok):
    assert ops.panel_linear16_supported(k, n_out, dt) is ok
