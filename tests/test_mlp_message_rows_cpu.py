"""The `mlp=True` part of the `half_messages` switch (ptgnn_amd/precision.py) without a GPU: set / restore semantics,
what `mlp_message_rows()` answers, and the CPU route of the MLP-MP layer rounding its messages under the switch."""
import pytest
import torch

import half_cases as C
import mlp_half_cases as MC


@pytest.fixture(autouse=True)
def restored():
    from ptgnn_amd import precision
    yield
    precision.set_matrix_inputs(torch.float32)
    precision.set_half_messages(False)


def test_keyword_sets_and_restores_both_parts():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert precision.get_half_messages_mlp() is False
    with ptgnn_amd.half_messages(mlp=True):
        assert precision.get_half_messages() is True and precision.get_half_messages_mlp() is True
        with ptgnn_amd.half_messages():                       # without the keyword: GGNN only
            assert precision.get_half_messages() is True and precision.get_half_messages_mlp() is False
        with ptgnn_amd.half_messages(False, mlp=True):        # off is off
            assert precision.get_half_messages() is False and precision.get_half_messages_mlp() is False
        assert precision.get_half_messages_mlp() is True
    assert precision.get_half_messages() is False and precision.get_half_messages_mlp() is False
    assert ptgnn_amd.set_half_messages(True, mlp=True) is False and precision.get_half_messages_mlp() is True
    assert ptgnn_amd.set_half_messages(True) is True and precision.get_half_messages_mlp() is False
    assert ptgnn_amd.set_half_messages(False) is True


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_mlp_message_rows_is_fp32_without_both_parts_and_on_the_cpu(dt):
    from ptgnn_amd import precision
    x = torch.zeros(2, 4)
    with precision.matrix_inputs(dt, mlp=True), precision.half_messages(mlp=True):
        assert precision.mlp_inputs(x) is dt and precision.mlp_message_rows(x) is torch.float32      # a CPU tensor

    class OnGpu:                                # what mlp_message_rows reads of a GPU tensor
        is_cuda, dtype = True, torch.float32
    with precision.matrix_inputs(dt, mlp=True):
        assert precision.mlp_message_rows(OnGpu) is torch.float32                                    # switch off
        with precision.half_messages():
            assert precision.mlp_message_rows(OnGpu) is torch.float32                                # GGNN part only
        with precision.half_messages(mlp=True):
            assert precision.mlp_message_rows(OnGpu) is dt
            OnGpu.dtype = dt
            assert precision.mlp_message_rows(OnGpu) is torch.float32                                # AMP states
            OnGpu.dtype = torch.float32
    with precision.matrix_inputs(dt), precision.half_messages(mlp=True):
        assert precision.mlp_message_rows(OnGpu) is torch.float32                                    # no mlp=True inputs


@pytest.mark.parametrize("use_dst", [True, False])
@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_route_rounds_each_message_once_under_the_switch(dt, use_dst):
    import ptgnn_amd
    F = torch.nn.functional
    torch.manual_seed(21)
    from ptgnn_amd import layers as L
    n, counts = 20, (17, 0, 30)
    layer = L.MlpMessagePassingLayer(32, 32, 32, len(counts), "sum", use_target_state_as_message_input=use_dst).eval()
    x, adj = torch.randn(n, 32), MC.adjacency(n, counts, 22)
    weights = layer.export_weights()
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt, mlp=True):
        off = MC.run_layer(layer, x, adj)
        with ptgnn_amd.half_messages():
            assert torch.equal(MC.run_layer(layer, x, adj), off)
        with ptgnn_amd.half_messages(mlp=True):
            on = MC.run_layer(layer, x, adj)
    with ptgnn_amd.matrix_inputs(dt, mlp=True), ptgnn_amd.half_messages(mlp=True):       # a gradient is needed: fp32
        with ptgnn_amd.matrix_inputs(torch.float32):
            fp32 = MC.run_layer(layer, x, adj)
        assert torch.equal(MC.run_layer(layer, x, adj), fp32)
    msgs = MC.messages64(x, adj, [w[0] for w in weights["edge_mlp"]], use_dst, dt).float().to(dt).double()
    agg = C.aggregate64(msgs, torch.cat([d for _, d in adj]), n, "sum")
    agg = F.layer_norm(F.gelu(agg), (32,), weights["ln_w"].double(), weights["ln_b"].double(), 1e-5)
    want = torch.tanh(agg @ weights["dense_w"].double().t() + weights["dense_b"].double())
    plain = MC.mlp64(x, adj, weights, dt=dt)
    assert C.err(off, plain) <= C.bar(plain) and not torch.equal(on, off)
    assert C.err(on, want) < C.err(on, plain) and C.err(on, want) < C.err(off, want)
