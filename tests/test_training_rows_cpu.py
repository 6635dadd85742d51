"""The `training` keyword of `set_half_messages` / `half_messages`, `precision.training_message_rows`, and the shape
predicates of the 16-bit training rows -- no GPU."""
import pytest
import torch

import ptgnn_amd
from ptgnn_amd import ops, precision

BF16 = torch.bfloat16


def test_keyword_semantics_and_nesting():
    gpu_like = torch.zeros(2, 32)                      # a CPU tensor: always float32 rows
    assert precision.training_message_rows(gpu_like) is torch.float32
    assert ptgnn_amd.set_half_messages(True, training=True) is False
    assert precision._half_messages_training and not precision.get_half_messages_mlp()
    assert ptgnn_amd.set_half_messages(True) is True and not precision._half_messages_training   # no keyword: off
    assert ptgnn_amd.set_half_messages(False, training=True) is True
    assert not precision._half_messages_training and not precision.get_half_messages()          # off is off
    with ptgnn_amd.half_messages(True, True):          # `mlp` stays the second positional parameter
        assert precision.get_half_messages_mlp() and not precision._half_messages_training
        with ptgnn_amd.half_messages(training=True):
            assert precision._half_messages_training and not precision.get_half_messages_mlp()
            with ptgnn_amd.half_messages():
                assert precision.get_half_messages() and not precision._half_messages_training
            assert precision._half_messages_training
        assert precision.get_half_messages_mlp() and not precision._half_messages_training
    assert not precision.get_half_messages()


def test_training_message_rows_needs_the_edge_training_setting_and_a_gpu_tensor(monkeypatch):
    cpu = torch.zeros(2, 32)
    with ptgnn_amd.half_messages(training=True):
        with ptgnn_amd.matrix_inputs(BF16, edge_training=True):
            assert precision.training_message_rows(cpu) is torch.float32
            monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # what a GPU tensor answers
            assert precision.training_message_rows(cpu) is BF16
            assert precision.training_message_rows(cpu.double()) is torch.float32
        with ptgnn_amd.matrix_inputs(BF16, edge_gemm=True, training=True):               # not edge_training
            assert precision.training_message_rows(cpu) is torch.float32
    with ptgnn_amd.half_messages(), ptgnn_amd.matrix_inputs(BF16, edge_training=True):   # not training=True
        assert precision.training_message_rows(cpu) is torch.float32


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_supported_twins_answer_without_a_device(dt):
    for fn in (ops.segment_reduce16_supported, ops.segment_spread16_supported):
        assert [fn(m, dt) for m in (32, 96, 256, 40, 288, 0)] == [True, True, True, False, False, False]
        assert not fn(64, torch.float32)
    takes = ops.edge_linear16_train_rows16_supported
    assert takes(64, 128, 3, dt, 1, False, True) and takes(128, 64, 3, dt, 2, True, True)
    assert takes(128, 64, 3, dt, 2, True, False) and takes(128, 64, 3, dt, 0, True, True)
    assert not takes(64, 128, 3, dt, 1, True, True) and not takes(64, 128, 3, dt, 2, False, True)
    assert not takes(64, 128, 3, dt, 1, False, False) and not takes(48, 128, 3, dt, 1, False, True)
    lib = ptgnn_amd._lib.load()
    assert lib.ptgnn_amd_edge_rows16_weight_grad16_supported(64, 128, 3, ops.HALF_IDS[dt]) == 1
    assert lib.ptgnn_amd_edge_rows16_weight_grad16_supported(64, 100, 3, ops.HALF_IDS[dt]) == 0
    names = ops.launch_counts(rows16=True)
    assert {"segment_reduce16", "segment_spread16", "edge16_train_rows16", "edge_wgrad16_rows16"} <= set(names)
