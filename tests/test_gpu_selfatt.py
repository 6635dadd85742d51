"""MultiHeadSelfAttentionMessagePassing on the MI355X: the fused block attention (csrc/block_attention.hip) against the
reference fixtures, a float64 restatement of selfattmessagepassing.py:104-117 at every tile boundary, peaked and flat
softmax rows, the hash dropout mask, determinism, the window table, AMP dtypes, a GGNN / attention / GGNN stack and the
no-score-matrix guarantee."""
import copy

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

from agg_paths import TOL, attributed_ok
from helpers import dropout_keep_scale
from ptgnn_amd import PtgnnAmdError, gnn as G, layers as L, ops
from segment_batches import ref_attention, window_offsets
from selfatt_cases import CASES, build, call, load

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def ok(got, want32, want64, what=""):
    """The attributed bar of tests/agg_paths.py, scaled by the largest float64 entry; prints each figure first."""
    want64 = torch.as_tensor(want64).detach().double().cpu()
    got64, w32 = got.detach().double().cpu(), torch.as_tensor(want32).detach().double().cpu()
    scale = max(1.0, float(want64.abs().max()))
    print(f"{what}: |got-fp32|={float((got64 - w32).abs().max()):.3e} |got-f64|={float((got64 - want64).abs().max()):.3e} "
          f"|fp32-f64|={float((w32 - want64).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, want64, tol=TOL, scale=scale)


def run_fixture(name, spec):
    fx = load(name)
    layer = build(spec, L).eval()
    layer.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}, strict=True)
    layer = layer.to(DEV)
    x = torch.from_numpy(fx["x"]).to(DEV).requires_grad_(True)
    y = call(layer, spec, x, fx["index"], fx.get("ids"), to=lambda t: t.to(DEV))
    y.backward(torch.from_numpy(fx["gout"]).to(DEV))
    got = {"y": y.detach(), "x": x.grad}
    got.update({k: p.grad.clone() for k, p in layer.named_parameters()})
    return fx, got


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    before = ops.launch_counts(aggregation=True)
    fx, got = run_fixture(name, spec)
    ran = ops.launches_since(before)
    assert ran.get("block_attention", 0) >= 1 and ran.get("block_attention_backward", 0) >= 1, ran
    assert ok(got["y"], fx["y"], fx["y64"], "y")
    for k in got:
        if k != "y":
            assert ok(got[k], fx["grad." + k], fx["grad64." + k], k), k


# ---------------------------------------------------------------------------------------------------------------------
# restatement of selfattmessagepassing.py:104-117 with a padded mask: windows as rows of a [W, L] batch
# (segment_batches.ref_attention / window_offsets), computed once per configuration
# ---------------------------------------------------------------------------------------------------------------------
REFS = {}


def reference(heads, dk, dv, counts, max_num_nodes, scale=1.0, p=0.0, seed=0, flat_window=False):
    """(kqv, gout, {dtype: (out, grad_kqv)}) on the CPU, computed once per configuration and never modified."""
    key = (heads, dk, dv, tuple(counts), max_num_nodes, scale, p, seed, flat_window)
    if key not in REFS:
        g = torch.Generator().manual_seed(900 + heads * 7 + dk * 3 + dv + len(counts))
        n = sum(counts)
        kqv = torch.randn(n, heads * (2 * dk + dv), generator=g) * scale
        if flat_window:                       # the first window: every score equal (all keys zero)
            kqv.reshape(n, heads, -1)[:counts[0], :, :dk] = 0.0
        gout = torch.randn(n, heads * dv, generator=g)
        mask = dropout_keep_scale(seed, n * heads, (max_num_nodes + 1) // 2 * 2, p) if p > 0 else None
        res = {}
        for dt in (torch.float32, torch.float64):
            k = kqv.to(dt).clone().requires_grad_(True)
            out = ref_attention(k, counts, max_num_nodes, heads, dk, dv, mask)
            out.backward(gout.to(dt))
            res[dt] = (out.detach(), k.grad)
        REFS[key] = (kqv, gout, res)
    return REFS[key]


def gpu_attention(kqv, gout, counts, max_num_nodes, heads, dk, dv, p=0.0, seed=0):
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(DEV)
    plan = ops.plan_for([(idx, idx)], len(counts))
    windows = ops.attention_windows(plan, max_num_nodes)
    kqv, gout = kqv.to(DEV), gout.to(DEV)
    out, lse = ops.block_attention(kqv, windows, max_num_nodes, heads, dk, dv, p, seed)
    grad = ops.block_attention_backward(kqv, out, lse, gout, windows, max_num_nodes, heads, dk, dv, p, seed)
    return out, grad, lse


MAXN = 130
TILES = sorted({ops.BLOCK_ATTENTION_COL_TILE, *ops.BLOCK_ATTENTION_ROW_TILES})
# window lengths 1, 2, max, (max + 1 -> max and 1), and one below / at / one above every tile size
COUNTS = [1, 2, MAXN, MAXN + 1, 0] + [t + d for t in TILES for d in (-1, 0, 1)]
SHAPES = [(1, 1, 1), (3, 6, 10), (8, 32, 32), (2, 64, 64), (1, 128, 128), (5, 33, 17)]


def test_tile_constants_and_case_size():
    assert TILES == [32, 64, 128] and sum(COUNTS) <= 1500
    assert MAXN > max(TILES) + 1


@pytest.mark.parametrize("heads,dk,dv", SHAPES, ids=[f"h{h}k{k}v{v}" for h, k, v in SHAPES])
def test_op_forward_and_backward_match_float64_at_every_tile_boundary(heads, dk, dv):
    kqv, gout, res = reference(heads, dk, dv, COUNTS, MAXN)
    before = ops.launch_counts(aggregation=True)
    out, grad, lse = gpu_attention(kqv, gout, COUNTS, MAXN, heads, dk, dv)
    assert ops.launches_since(before) == {"block_attention": 1, "block_attention_backward": 1}
    assert out.shape == (kqv.shape[0], heads * dv) and lse.shape == (kqv.shape[0], heads)
    assert ok(out, res[torch.float32][0], res[torch.float64][0], "out")
    assert ok(grad, res[torch.float32][1], res[torch.float64][1], "grad_kqv")


def test_small_max_num_nodes_cuts_graphs_into_many_windows():
    counts = [40, 1, 0, 41, 87, 2, 65]
    kqv, gout, res = reference(3, 6, 10, counts, 40)
    out, grad, _ = gpu_attention(kqv, gout, counts, 40, 3, 6, 10)
    assert ok(out, res[torch.float32][0], res[torch.float64][0], "out")
    assert ok(grad, res[torch.float32][1], res[torch.float64][1], "grad_kqv")


def test_peaked_and_flat_softmax_rows_stay_finite_and_on_the_bar():
    counts = [70, 33, MAXN, 65]
    kqv, gout, res = reference(4, 16, 16, counts, MAXN, scale=30.0, flat_window=True)
    out, grad, lse = gpu_attention(kqv, gout, counts, MAXN, 4, 16, 16)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(lse).all())
    probs_max = torch.softmax(torch.einsum("khd,vhd->khv", kqv[70:103].reshape(33, 4, -1)[..., :16].double(),
                                           kqv[70:103].reshape(33, 4, -1)[..., 16:32].double()) / 4.0, -1).amax(-1)
    assert float(probs_max.median()) > 0.99                        # rows of the second window are nearly one-hot
    assert ok(out, res[torch.float32][0], res[torch.float64][0], "out")
    flat = lse[:70].cpu().double()                                  # all scores 0: lse = log(70), out = the mean value
    assert float((flat - np.log(70.0)).abs().max()) < 1e-5


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_the_hash_mask_at_the_op(p):
    counts, seed = [40, 1, 0, 41, 87, 2, 65], (5 << 40) + 1234
    kqv, gout, res = reference(3, 6, 10, counts, 41, p=p, seed=seed)        # odd max_num_nodes: W = 42
    out, grad, _ = gpu_attention(kqv, gout, counts, 41, 3, 6, 10, p, seed)
    assert ok(out, res[torch.float32][0], res[torch.float64][0], "out")
    assert ok(grad, res[torch.float32][1], res[torch.float64][1], "grad_kqv")
    plain = reference(3, 6, 10, counts, 41)[2][torch.float64][0]
    assert float((out.cpu().double() - plain).abs().max()) > 1e-2            # the mask did something


def test_zero_dropout_rate_equals_the_entry_without_dropout_bit_for_bit():
    kqv, gout, _ = reference(3, 6, 10, COUNTS, MAXN)
    a = gpu_attention(kqv, gout, COUNTS, MAXN, 3, 6, 10)
    b = gpu_attention(kqv, gout, COUNTS, MAXN, 3, 6, 10, 0.0, 987654321)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_two_runs_give_the_same_bits_and_a_graph_does_not_depend_on_its_batch():
    name, spec = CASES[0]
    _, first = run_fixture(name, spec)
    _, second = run_fixture(name, spec)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    kqv, gout, _ = reference(8, 32, 32, COUNTS, MAXN)
    out, grad, _ = gpu_attention(kqv, gout, COUNTS, MAXN, 8, 32, 32)
    lo = sum(COUNTS[:3])                                             # the MAXN + 1 graph: two windows
    alone = gpu_attention(kqv[lo:lo + MAXN + 1], gout[lo:lo + MAXN + 1], [MAXN + 1], MAXN, 8, 32, 32)
    assert torch.equal(out[lo:lo + MAXN + 1], alone[0]) and torch.equal(grad[lo:lo + MAXN + 1], alone[1])


def test_window_table_of_an_unsorted_map_with_empty_graphs():
    counts = [5, 0, 0, 12, 1, 0, 9, 4, 0]
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    idx = idx[torch.randperm(idx.shape[0], generator=torch.Generator().manual_seed(3))]
    assert not bool((idx[1:] >= idx[:-1]).all())
    n, G_ = idx.shape[0], len(counts)
    for max_nodes in (1, 4, 5, 250):
        d = idx.to(DEV)
        table = ops.attention_windows(ops.plan_for([(d, d)], G_), max_nodes).cpu().numpy()
        want = window_offsets(np.bincount(idx.numpy(), minlength=G_).tolist(), max_nodes)
        bound = -(-n // max_nodes) + G_
        assert table.shape == (bound + 1,) and table.dtype == np.int32
        assert table[:len(want)].tolist() == want and (table[len(want):] == n).all()


def make_layer(D=64, dk=16, dv=24, heads=4, inter=96, p=0.0, max_num_nodes=50, seed=5):
    torch.manual_seed(seed)
    return L.MultiHeadSelfAttentionMessagePassing(D, dk, dv, D, inter, heads, dropout_rate=p, max_num_nodes=max_num_nodes)


def test_training_with_dropout_launches_both_families_and_differs_from_eval(monkeypatch):
    monkeypatch.setattr(L, "_dropout_seed", lambda: 424242)
    layer = make_layer(p=0.1).to(DEV)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(333, 64, generator=g).to(DEV).requires_grad_(True)
    idx = torch.repeat_interleave(torch.arange(4), torch.tensor([120, 1, 150, 62])).to(DEV)
    layer.train()
    before = ops.launch_counts(aggregation=True)
    y = layer(x, [], idx, {}, {}, [])
    y.sum().backward()
    ran = ops.launches_since(before)
    assert ran.get("block_attention") == 1 and ran.get("block_attention_backward") == 1, ran
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in layer.parameters())
    with torch.no_grad():
        y_eval = layer.eval()(x, [], idx, {}, {}, [])
    assert float((y.detach() - y_eval).abs().max()) > 1e-3


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_keep_their_dtype_and_equal_the_fp32_route(dtype):
    layer = make_layer().to(DEV).eval()
    x = torch.randn(200, 64, generator=torch.Generator().manual_seed(7)).to(DEV).to(dtype)
    idx = torch.repeat_interleave(torch.arange(3), torch.tensor([120, 1, 79])).to(DEV)
    with torch.no_grad():
        y = layer(x, [], idx, {}, {}, [])
        y32 = layer(x.float(), [], idx, {}, {}, [])
    assert y.dtype == dtype and y32.dtype == torch.float32 and torch.equal(y, y32.to(dtype))


def test_unsupported_dimensions_raise():
    idx = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(PtgnnAmdError, match="128"):
        L.MultiHeadSelfAttentionMessagePassing(16, 129, 8, 16, 16, 1).to(DEV)(torch.randn(8, 16, device=DEV), [], idx, {}, {}, [])
    with pytest.raises(PtgnnAmdError, match="512"):
        L.MultiHeadSelfAttentionMessagePassing(516, 8, 8, 516, 16, 1).to(DEV)(torch.randn(8, 516, device=DEV), [], idx, {}, {}, [])


class _Embed(nn.Module):
    def forward(self, x):
        return x


def test_ggnn_attention_ggnn_stack_eval_and_training_step_match_the_cpu_route():
    H, T = 64, 2
    torch.manual_seed(7)
    net = G.GraphNeuralNetwork([L.GatedMessagePassingLayer(H, H, 2 * T + 1, "sum"),
                                L.MultiHeadSelfAttentionMessagePassing(H, 16, 16, H, 96, 4, max_num_nodes=100),
                                L.GatedMessagePassingLayer(H, H, 2 * T + 1, "max")], _Embed(),
                               introduce_backwards_edges=True, add_self_edges=True)
    g = torch.Generator().manual_seed(8)
    sizes = [300, 1, 150, 40, 2]
    N = sum(sizes)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    lo = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0)[idx]    # edges stay inside their graph
    span = torch.tensor(sizes)[idx]
    adj = []
    for _ in range(T):
        src = torch.randint(0, N, (3 * N,), generator=g)
        dst = lo[src] + torch.randint(0, 1 << 30, (3 * N,), generator=g) % span[src]
        adj.append((src, dst))
    x = torch.randn(N, H, generator=g)
    gout = torch.randn(N, H, generator=g)

    def run(module, dev, dt, train):
        module.train(train)
        module.zero_grad(set_to_none=True)
        xr = x.detach().to(dev, dt).clone().requires_grad_(train)
        out = module(node_data={"x": xr}, adjacency_lists=[(s.to(dev), d.to(dev)) for s, d in adj], edge_feature_data=[],
                     node_to_graph_idx=idx.to(dev), reference_node_ids={}, reference_node_graph_idx={},
                     num_graphs=len(sizes)).output_node_representations
        res = {"y": out.detach()}
        if train:
            out.backward(gout.to(dev, dt))
            res["x"] = xr.grad
            res.update({k: p.grad.clone() for k, p in module.named_parameters()})
        return res

    cpu = {dt: copy.deepcopy(net).to(dt) for dt in (torch.float32, torch.float64)}
    gpu = net.to(DEV)
    for train in (False, True):
        with (torch.enable_grad() if train else torch.no_grad()):
            before = ops.launch_counts(aggregation=True)
            got = run(gpu, DEV, torch.float32, train)
            ran = ops.launches_since(before)
            want = {dt: run(m, "cpu", dt, train) for dt, m in cpu.items()}
        assert ran.get("block_attention") == 1 and ran.get("block_attention_backward", 0) == (1 if train else 0), ran
        assert set(got) == set(want[torch.float64])
        for k, v in got.items():
            assert ok(v, want[torch.float32][k], want[torch.float64][k], f"train={train} {k}"), (train, k)


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.shapes = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.shapes += [(func.overloadpacket.__name__, tuple(t.shape)) for t in outs if isinstance(t, torch.Tensor)]
        return out


def test_inference_creates_no_score_matrix():
    N, maxn = 20_000, 250
    layer = make_layer(max_num_nodes=maxn).to(DEV).eval()
    x = torch.randn(N, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    idx = torch.repeat_interleave(torch.arange(8), N // 8).to(DEV)
    with torch.no_grad():
        layer(x, [], idx, {}, {}, [])                              # plan and graph count warmed
        before = ops.launch_counts(aggregation=True)
        with _Recorder() as rec:
            y = layer(x, [], idx, {}, {}, [])
        ran = ops.launches_since(before)
    assert ran.get("block_attention") == 1 and "block_attention_backward" not in ran, ran
    assert y.shape == (N, 64) and bool(torch.isfinite(y).all())
    per_graph = N // 8
    for name, shape in rec.shapes:
        assert not (len(shape) >= 2 and shape[-1] in (maxn, per_graph, N) and shape[-2] in (maxn, per_graph, N)), (name, shape)
        assert not (len(shape) >= 2 and shape[0] == N and shape[-1] == maxn), (name, shape)
        assert int(np.prod(shape)) <= N * max(64, 96, 4 * (2 * 16 + 24)), (name, shape)
