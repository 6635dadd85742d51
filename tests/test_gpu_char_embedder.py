"""CharUnitEmbedder on the MI355X: the char-embed table sum, the windowed GEMMs over row frames and the window max
(csrc/char_conv.hip, ptgnn_amd/char_cnn.py) against the reference fixtures and against a float64 restatement at every
batch size, window combination and width class; sample isolation (no valid row reads a junk or pad row), the exact cases
(a selection, one gradient row per column, the lowest tied position), determinism across the backward's chunks, and
dispatch (launch counters, the composed route, AMP dtypes, the module as the node embedder of a GraphNeuralNetwork)."""
import contextlib
from unittest import mock

import pytest
import torch
from torch import nn

from agg_paths import TOL, attributed_ok
from char_embedder_cases import CASES, PARAMS, build, load, make_chars, reference, state_of
from ptgnn_amd import PtgnnAmdError, embeddings, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXTURE_TOL = 2e-5          # the bar of tests/test_gpu_embedder.py, relative to max(1, max |want|)
GRAD_TOL = 2e-5             # DESIGN section 6, relative to max |g|
ALL_COUNTERS = dict(aggregation=True, char_cnn=True)
CHAR_LAUNCHES = {"char_embed": 1, "char_embed_backward": 1, "window_max": 1, "window_max_backward": 1}


def _refuse(name):
    def raiser(*args, **kwargs):
        raise AssertionError(f"{name} was called on the GPU route")
    return raiser


@contextlib.contextmanager
def no_vendor_calls():
    with mock.patch.object(nn.functional, "conv1d", _refuse("F.conv1d")), \
            mock.patch.object(nn.functional, "one_hot", _refuse("F.one_hot")), \
            mock.patch.object(nn.functional, "linear", _refuse("F.linear")), \
            mock.patch.object(nn.functional, "embedding", _refuse("F.embedding")):
        yield


def char_launches(since):
    return {k: v for k, v in since.items() if k in CHAR_LAUNCHES}


def attributed(got, want32, exact, what):
    """The attributed rule of tests/agg_paths.py scaled by max(1, max |float64|)."""
    got, want32, exact = got.detach().cpu(), want32.detach().cpu(), exact.detach().cpu()
    scale = max(1.0, float(exact.abs().max()))
    print(f"    {what}: |got-fp32|={float((got - want32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


def make_module(C, L, widths, windows, seed):
    F1, F2, D = widths
    k1, k2, k3 = windows
    torch.manual_seed(seed)
    return embeddings.CharUnitEmbedder(C, D, embeddings.CnnConfig(F1, k1, F2, k2, k3))


def params_of(module):
    named = dict(module.named_parameters())
    return [named[k] for k in PARAMS]


def run(module, chars, coef):
    """(out, [d param ...]) of one forward + backward of sum(out * coef) on the GPU; the gradients are cleared first."""
    module.zero_grad(set_to_none=True)
    out = module(chars)
    (out * coef).sum().backward()
    return out.detach(), [p.grad.clone() for p in params_of(module)]


def against_float64(module, chars, coef, what):
    cpu_params = [p.detach().cpu() for p in params_of(module)]
    o32, g32 = reference(chars, cpu_params, coef, torch.float32)
    o64, g64 = reference(chars, cpu_params, coef, torch.float64)
    with no_vendor_calls():
        out, grads = run(module, chars.to(DEV), coef.to(DEV))
    assert attributed(out, o32, o64, f"{what} out"), what
    for k, g, a, b in zip(PARAMS, grads, g32, g64):
        assert attributed(g, a, b, f"{what} d {k.split('__')[1]}"), (what, k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    fx = load(name)
    module = build(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    module = module.to(DEV)
    chars, coef = torch.from_numpy(fx["chars"]).to(DEV), torch.from_numpy(fx["coef"]).to(DEV)
    before = ops.launch_counts(**ALL_COUNTERS)
    with no_vendor_calls():
        out = module(chars)
        (out * coef).sum().backward()
    since = char_launches(ops.launches_since(before))
    if name == "charcnn_odd":                                     # the composed route: no char-embed kernel
        assert since == {"window_max": 1, "window_max_backward": 1}
    else:
        assert since == CHAR_LAUNCHES
    want = torch.from_numpy(fx["out"])
    err, scale = float((out.detach().cpu() - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"    out: |got - want| = {err:.3e} (scale {scale:.3e})")
    assert err <= FIXTURE_TOL * scale
    for k, p in module.named_parameters():
        g = torch.from_numpy(fx["grad." + k])
        err = float((p.grad.cpu() - g).abs().max())
        print(f"    {k}: |got - want| = {err:.3e} (max |g| {float(g.abs().max()):.3e})")
        assert err <= GRAD_TOL * float(g.abs().max()), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. the sweep against float64
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((7, (3, 3, 3)), (15, (3, 3, 3)), (5, (1, 1, 5)), (11, (2, 4, 3)))


@pytest.mark.parametrize("widths", ((8, 4, 4), (64, 32, 64)), ids=("w8_4_4", "w64_32_64"))
@pytest.mark.parametrize("L,windows", SHAPES, ids=[f"L{L}_k{''.join(map(str, k))}" for L, k in SHAPES])
def test_sweep_against_float64(L, windows, widths):
    C = 13
    module = make_module(C, L, widths, windows, seed=100 * L + widths[0]).to(DEV)
    assert ops.char_embed_supported(C, windows[0], widths[0])
    for B in (1, 3, 257):
        gen = torch.Generator().manual_seed(1000 * L + 10 * widths[0] + B)
        chars = make_chars(B, L, C, gen, padded=(B == 3))
        coef = torch.randn(B, widths[2], generator=gen)
        before = ops.launch_counts(**ALL_COUNTERS)
        against_float64(module, chars, coef, f"B={B}")
        assert char_launches(ops.launches_since(before)) == CHAR_LAUNCHES


def test_default_configuration_against_float64():
    """CnnConfig(256, 3, 128, 3, 3), 70 characters, 15 chars per string, embedding size 128 -- the reference's defaults."""
    B, L, C = 3, 15, 70
    module = make_module(C, L, (256, 128, 128), (3, 3, 3), seed=7).to(DEV)
    gen = torch.Generator().manual_seed(70)
    chars, coef = make_chars(B, L, C, gen), torch.randn(B, 128, generator=gen)
    before = ops.launch_counts(**ALL_COUNTERS)
    against_float64(module, chars, coef, "default")
    assert char_launches(ops.launches_since(before)) == CHAR_LAUNCHES


@pytest.mark.parametrize("C", (86, 100, 213))
def test_char_tables_whose_backward_tile_needs_the_lds_opt_in_against_float64(C):
    """k1 = 3: from 86 characters on, the backward's (3 C + 1) x 64-float table tile is beyond the 64 KiB a kernel gets
    without the dynamic-LDS opt-in; 213 characters make it exactly the 160 KiB of a CU, the last supported size."""
    assert (3 * C + 1) * 256 > 64 * 1024 and ops.char_embed_supported(C, 3, 8) and not ops.char_embed_supported(214, 3, 8)
    B, L = 37, 9
    module = make_module(C, L, (8, 4, 4), (3, 3, 3), seed=C).to(DEV)
    gen = torch.Generator().manual_seed(C + 1)
    chars, coef = make_chars(B, L, C, gen), torch.randn(B, 4, generator=gen)
    chars[0, :4] = torch.tensor([0, C - 1, C - 1, 0])                       # the first and the last table row of every tap
    before = ops.launch_counts(**ALL_COUNTERS)
    against_float64(module, chars, coef, f"C={C}")
    assert char_launches(ops.launches_since(before)) == CHAR_LAUNCHES


def test_windowed_gemms_on_the_streaming_kernels_against_float64(monkeypatch):
    """PTGNN_AMD_FORCE_STREAM=1 lifts the size thresholds of the streaming Linear, so the overlapping rows go through its
    operand loads as well as through the tile kernel's (which the small shapes above take)."""
    monkeypatch.setenv("PTGNN_AMD_FORCE_STREAM", "1")
    B, L, C = 257, 15, 13
    module = make_module(C, L, (64, 32, 64), (3, 3, 3), seed=11).to(DEV)
    gen = torch.Generator().manual_seed(12)
    chars, coef = make_chars(B, L, C, gen), torch.randn(B, 64, generator=gen)
    before = ops.launch_counts(**ALL_COUNTERS)
    against_float64(module, chars, coef, "forced stream")
    since = ops.launches_since(before)
    assert since.get("k_stream_linear", 0) >= 2, since


# ---------------------------------------------------------------------------------------------------------------------
# 3. sample isolation: no valid row reads a junk row, a pad row or another sample's row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("changed", ("middle", "last"))
def test_changing_one_sample_leaves_every_other_sample_bit_identical(changed):
    B, L, C, widths, windows = 7, 11, 13, (16, 8, 8), (2, 4, 3)
    module = make_module(C, L, widths, windows, seed=21).to(DEV)
    gen = torch.Generator().manual_seed(22)
    chars = make_chars(B, L, C, gen)
    victim = B // 2 if changed == "middle" else B - 1
    other = chars.clone()
    other[victim] = (chars[victim] + 1 + torch.arange(L)) % C
    assert not torch.equal(other[victim], chars[victim])
    keep = [b for b in range(B) if b != victim]
    for lit in sorted({victim - 1, min(victim + 1, B - 2), 0}):
        coef = torch.zeros(B, widths[2])
        coef[lit] = torch.randn(widths[2], generator=gen)       # only sample `lit` (not the victim) reaches the loss
        out_a, grads_a = run(module, chars.to(DEV), coef.to(DEV))
        out_b, grads_b = run(module, other.to(DEV), coef.to(DEV))
        assert torch.equal(out_a[keep], out_b[keep]) and not torch.equal(out_a[victim], out_b[victim])
        for k, a, b in zip(PARAMS, grads_a, grads_b):
            assert bool(a.any()) and torch.equal(a, b), (lit, k)


# ---------------------------------------------------------------------------------------------------------------------
# 4. exactness that follows from the arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_unit_windows_and_identity_weights_make_the_output_a_selection():
    B, L, C, F = 37, 9, 13, 8
    module = make_module(C, L, (F, F, F), (1, 1, 1), seed=31)
    w1, b1, w2, b2, w3 = params_of(module)
    with torch.no_grad():
        b1.zero_()
        b2.zero_()
        w2.copy_(torch.eye(F).unsqueeze(-1))
        w3.copy_(torch.eye(F).unsqueeze(-1))
    chars = make_chars(B, L, C, torch.Generator().manual_seed(32))
    want = torch.relu(w1.detach()[:, :, 0].t()[chars]).max(dim=1)[0]          # the max over positions of table rows
    with torch.no_grad(), no_vendor_calls():
        got = module.to(DEV)(chars.to(DEV))
    assert torch.equal(got.cpu(), want)


def test_window_max_takes_the_lowest_tied_position_and_its_backward_fills_one_row_per_column():
    fx, spec = load("charcnn_padded"), dict(CASES)["charcnn_padded"]
    state = state_of(fx)
    w1, b1 = state[PARAMS[0]].to(DEV), state[PARAMS[1]].to(DEV)
    k1, C, B = spec["k"][0], spec["C"], spec["B"]
    chars = torch.from_numpy(fx["chars"]).to(DEV)
    R = spec["L"] - k1 + 1
    a1 = ops.char_embed(chars, w1.permute(2, 1, 0).reshape(k1 * C, -1).contiguous(), b1, k1)    # repeated windows: ties
    D = a1.shape[1]
    for valid in (R, R - 4, 1):
        out, arg = ops.window_max(a1, 0, B, R, valid, return_arg=True)
        x = a1.reshape(B, R, D)[:, :valid].cpu()
        best = x.max(dim=1)[0]
        first = (x == best.unsqueeze(1)).int().argmax(dim=1)                # the lowest position that attains the maximum
        ties = ((x == best.unsqueeze(1)).sum(dim=1) > 1)
        assert valid == 1 or bool(ties.any())
        assert torch.equal(out.cpu(), best) and torch.equal(arg.cpu().long(), first)
        g = torch.randn(B, D, device=DEV) + 3.0                            # no zero entry
        gx = ops.window_max_backward(g, arg, R).reshape(B, R, D)
        assert torch.equal((gx != 0).sum(dim=1), torch.ones(B, D, dtype=torch.int64, device=DEV))
        assert torch.equal(gx.gather(1, arg.long().unsqueeze(1)).squeeze(1), g)
        assert not gx[:, valid:].any()


def test_char_embed_clamps_ids_outside_the_table():
    C, k1, F = 5, 2, 8
    table, bias = torch.randn(k1 * C, F, device=DEV), torch.randn(F, device=DEV)
    chars = torch.tensor([[0, -3, 4, 99, 2]], device=DEV)
    got = ops.char_embed(chars, table, bias, k1, act=None)
    want = ops.char_embed(chars.clamp(0, C - 1), table, bias, k1, act=None)
    assert torch.equal(got, want)
    g = torch.randn(4, F, device=DEV)
    for a, b in zip(ops.char_embed_backward(g, None, chars, C, k1, act=None),
                    ops.char_embed_backward(g, None, chars.clamp(0, C - 1), C, k1, act=None)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism across the backward's chunks
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits_across_backward_chunks():
    chunk = ops.char_embed_backward_chunk()
    B, L, C = 3 * chunk + 1, 7, 13                                          # three full chunks and one sample
    module = make_module(C, L, (8, 4, 4), (3, 3, 3), seed=41).to(DEV)
    gen = torch.Generator().manual_seed(42)
    chars, coef = make_chars(B, L, C, gen).to(DEV), torch.randn(B, 4, generator=gen).to(DEV)
    first = run(module, chars, coef)
    second = run(module, chars, coef)
    assert torch.equal(first[0], second[0])
    for k, a, b in zip(PARAMS, first[1], second[1]):
        assert bool(a.any()) and torch.equal(a, b), k
    # the chunked table gradient against float64, the last chunk holding a single sample
    cpu_params = [p.detach().cpu() for p in params_of(module)]
    _, g32 = reference(chars, cpu_params, coef, torch.float32)
    _, g64 = reference(chars, cpu_params, coef, torch.float64)
    for k, g, a, b in zip(PARAMS, first[1], g32, g64):
        assert attributed(g, a, b, f"d {k.split('__')[1]}"), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_composed_route_for_odd_widths_matches_float64_without_a_char_embed_launch():
    spec = dict(CASES)["charcnn_odd"]
    B, L, C = 37, spec["L"], spec["C"]
    module = make_module(C, L, (spec["F1"], spec["F2"], spec["D"]), tuple(spec["k"]), seed=51).to(DEV)
    gen = torch.Generator().manual_seed(52)
    chars, coef = make_chars(B, L, C, gen), torch.randn(B, spec["D"], generator=gen)
    before = ops.launch_counts(**ALL_COUNTERS)
    against_float64(module, chars, coef, "odd")
    assert char_launches(ops.launches_since(before)) == {"window_max": 1, "window_max_backward": 1}


def test_inference_makes_one_char_embed_and_one_window_max_launch():
    module = make_module(13, 15, (16, 8, 8), (3, 3, 3), seed=61).to(DEV).eval()
    chars = make_chars(50, 15, 13, torch.Generator().manual_seed(62)).to(DEV)
    before = ops.launch_counts(**ALL_COUNTERS)
    with torch.no_grad(), no_vendor_calls():
        out = module(chars)
    assert tuple(out.shape) == (50, 8)
    assert char_launches(ops.launches_since(before)) == {"char_embed": 1, "window_max": 1}


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_half_parameters_round_trip_their_dtype(dtype):
    chars = make_chars(20, 15, 13, torch.Generator().manual_seed(71)).to(DEV)
    half = make_module(13, 15, (16, 8, 8), (3, 3, 3), seed=72).to(DEV).to(dtype)
    full = make_module(13, 15, (16, 8, 8), (3, 3, 3), seed=72).to(DEV)
    full.load_state_dict({k: v.float() for k, v in half.state_dict().items()})
    out = half(chars)
    out.float().sum().backward()
    assert out.dtype == dtype and all(p.grad is not None and p.grad.dtype == dtype for p in half.parameters())
    with torch.no_grad():
        assert torch.equal(out.detach(), full(chars).to(dtype))


def test_bad_inputs_raise():
    module = make_module(13, 15, (16, 8, 8), (3, 3, 3), seed=81).to(DEV)
    with pytest.raises(PtgnnAmdError, match="fewer than the 7"):
        module(torch.zeros(2, 6, dtype=torch.int64, device=DEV))
    with pytest.raises(PtgnnAmdError, match="CUDA int64"):
        module(torch.zeros(2, 9, dtype=torch.int32, device=DEV))
    with pytest.raises(PtgnnAmdError, match="CUDA int64"):
        module(torch.zeros(2, 9, dtype=torch.int64))
    frame = torch.zeros(10, 8, device=DEV)
    with pytest.raises(PtgnnAmdError, match="reach outside"):
        ops.window_linear(frame, 0, 9, 3, torch.zeros(4, 24, device=DEV))     # the last window would end past the frame
    with pytest.raises(PtgnnAmdError, match="contiguous"):
        ops.window_linear(frame.as_strided((8, 24), (8, 1)), 0, 8, 1, torch.zeros(4, 24, device=DEV))


def test_node_embedder_of_a_two_layer_ggnn():
    from ptgnn_amd import layers as L, workloads
    from ptgnn_amd.gnn import GraphNeuralNetwork
    mb = workloads.batched_graphs(3, 60, 3, 2.2, seed=3)
    N, H, T, C = mb["num_nodes"], 64, 7, 30
    torch.manual_seed(0)
    embedder = embeddings.CharUnitEmbedder(C, H, embeddings.CnnConfig(32, 3, 16, 3, 3))
    node_data = {"chars": make_chars(N, 15, C, torch.Generator().manual_seed(4), padded=True).to(DEV)}
    net = GraphNeuralNetwork([L.GatedMessagePassingLayer(H, H, T, "max"), L.GatedMessagePassingLayer(H, H, T, "sum")],
                             embedder, True, True).to(DEV)
    before = ops.launch_counts(**ALL_COUNTERS)
    with mock.patch.object(nn.functional, "conv1d", _refuse("F.conv1d")), \
            mock.patch.object(nn.functional, "one_hot", _refuse("F.one_hot")), \
            mock.patch.object(nn.functional, "embedding", _refuse("F.embedding")):
        out = net(node_data=node_data, adjacency_lists=[(s.to(DEV), d.to(DEV)) for s, d in mb["adjacency_lists"]],
                  edge_feature_data=[], node_to_graph_idx=mb["node_to_graph_idx"].to(DEV),
                  reference_node_ids={k: v.to(DEV) for k, v in mb["reference_node_ids"].items()},
                  reference_node_graph_idx={k: v.to(DEV) for k, v in mb["reference_node_graph_idx"].items()},
                  num_graphs=mb["num_graphs"])
        states = out.output_node_representations
        states.square().sum().backward()
    assert char_launches(ops.launches_since(before)) == CHAR_LAUNCHES
    assert tuple(states.shape) == (N, H) and bool(torch.isfinite(states).all())
    for p in embedder.parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.any())
