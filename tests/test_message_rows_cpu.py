"""The `half_messages` switch of ptgnn_amd/precision.py without a GPU: its defaults, nesting and restore, its
independence from `set_matrix_inputs`, what `message_rows()` answers for every combination, and the CPU route of the
GGNN layer rounding its messages under the switch, in inference only."""
import itertools

import pytest
import torch

import half_cases as C

SETTINGS = (torch.float32, torch.bfloat16, torch.float16, "autocast")


@pytest.fixture(autouse=True)
def restored():
    from ptgnn_amd import precision
    yield
    precision.set_matrix_inputs(torch.float32)
    precision.set_half_messages(False)


def test_switch_defaults_nesting_and_independence():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.get_half_messages() is False and ptgnn_amd.set_half_messages is precision.set_half_messages
    with ptgnn_amd.half_messages():
        assert precision.get_half_messages() is True
        with ptgnn_amd.half_messages(False):
            assert precision.get_half_messages() is False
        assert precision.get_half_messages() is True
        # set_matrix_inputs / matrix_inputs neither read nor reset the switch ...
        precision.set_matrix_inputs(torch.float32)
        with precision.matrix_inputs(torch.bfloat16, edge_gemm=True):
            assert precision.get_half_messages() is True
        assert precision.get_half_messages() is True
    assert precision.get_half_messages() is False
    assert ptgnn_amd.set_half_messages(True) is False and ptgnn_amd.set_half_messages(False) is True
    # ... and the switch leaves the matrix-input setting and its flags alone
    precision.set_matrix_inputs(torch.float16, edge_gemm=True)
    with precision.half_messages():
        pass
    x = torch.zeros(2, 4)
    assert precision.get_matrix_inputs() is torch.float16 and precision.edge_gemm_inputs(x) is torch.float16


@pytest.mark.parametrize("on,edge_gemm,setting", list(itertools.product((False, True), (False, True), SETTINGS)))
def test_message_rows_for_every_combination(on, edge_gemm, setting):
    from ptgnn_amd import precision
    x = torch.zeros(2, 4)                      # a CPU tensor: "autocast" resolves to float32 for it
    resolved = setting if isinstance(setting, torch.dtype) else torch.float32
    with precision.matrix_inputs(setting, edge_gemm=edge_gemm), precision.half_messages(on):
        assert precision.message_rows(x, edge_form=False) is (resolved if on else torch.float32)
        assert precision.message_rows(x, edge_form=True) is (resolved if on and edge_gemm else torch.float32)


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_route_rounds_messages_under_the_switch_in_inference_only(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    n, counts = 60, (40, 0, 25)
    torch.manual_seed(11)
    layer = L.GatedMessagePassingLayer(32, 32, len(counts), "sum").eval()
    x, adj = torch.randn(n, 32), C.random_adjacency(n, counts, 12)
    feats = [torch.empty(c, 0) for c in counts]
    weights = layer.export_weights()

    def run():
        return layer(x, adj, None, {}, {}, feats)
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt):
        off = run()
        with ptgnn_amd.half_messages():
            on = run()
    msgs = torch.cat([C.linear64(x, w, dt=dt)[s] for (s, _), w in zip(adj, weights["edge_w"])])
    agg = C.aggregate64(msgs.float().to(dt).double(), torch.cat([d for _, d in adj]), n, "sum")
    want = C.gru64(agg.float(), x, weights["w_ih"], weights["w_hh"], weights["b_ih"], weights["b_hh"], dt=dt)
    plain, _ = C.ggnn64(x, adj, weights, linear_dt=dt, gru_dt=dt)
    assert C.err(off, plain) <= 4 * C.bar(plain) and not torch.equal(on, off)
    assert C.err(on, want) < C.err(on, plain) and C.err(on, want) < C.err(off, want)
    with ptgnn_amd.half_messages():
        with torch.no_grad():
            fp32 = run()                        # float32 setting: the switch means fp32 rows
            with ptgnn_amd.matrix_inputs(torch.float32):
                assert torch.equal(run(), fp32)
        with ptgnn_amd.matrix_inputs(dt):       # a gradient is needed: nothing is rounded
            assert torch.equal(run().detach(), fp32)
