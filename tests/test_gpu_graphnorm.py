"""GraphNorm on the MI355X: the fused HIP kernels (csrc/graph_norm.hip) against the reference fixtures, a float64
restatement of graphnorm.py:36-46 at D in {6, 64, 100, 256, 512, 1024} up to the Graph2Class scale, the 128-row chunk
boundaries, the composed route beyond D = 1024, determinism, the no-[N, D]-intermediate guarantee, AMP dtypes and a
GGNN / GraphNorm / GGNN stack."""
import copy
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

from agg_paths import TOL, attributed_ok
from graphnorm_cases import CASES, build
from ptgnn_amd import gnn as G, layers as L, ops
from segment_batches import ref_graphnorm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
PARAMS = ("gamma", "alpha", "bias")


def load(name):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return {k: z[k] for k in z.files}


def ok(got, want32, want64, what=""):
    """The attributed bar of tests/agg_paths.py, scaled by the largest float64 entry; prints each figure first."""
    want64 = torch.as_tensor(want64).detach().double().cpu()
    got64, w32 = got.detach().double().cpu(), torch.as_tensor(want32).detach().double().cpu()
    scale = max(1.0, float(want64.abs().max()))
    print(f"{what}: |got-fp32|={float((got64 - w32).abs().max()):.3e} |got-f64|={float((got64 - want64).abs().max()):.3e} "
          f"|fp32-f64|={float((w32 - want64).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, want64, tol=TOL, scale=scale)


def run_layer(layer, x, idx, gout):
    layer.zero_grad(set_to_none=True)
    xr = x.detach().clone().requires_grad_(True)
    y = layer(xr, [], idx, {}, {}, [])
    y.backward(gout)
    out = {"y": y.detach(), "x": xr.grad}
    out.update({k: getattr(layer, k).grad.clone() for k in PARAMS})
    return out


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    fx = load(name)
    layer = build(spec, L)
    layer.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}, strict=True)
    layer = layer.to(DEV)
    before = ops.launch_counts(aggregation=True)
    got = run_layer(layer, torch.from_numpy(fx["x"]).to(DEV), torch.from_numpy(fx["index"]).to(DEV),
                    torch.from_numpy(fx["gout"]).to(DEV))
    ran = ops.launches_since(before)
    assert ran.get("graph_norm", 0) >= 1 and ran.get("graph_norm_backward", 0) >= 1, ran
    assert ok(got["y"], fx["y"], fx["y64"], "y")
    for k in ("x",) + PARAMS:
        assert ok(got[k], fx["grad." + k], fx["grad64." + k], k), k


# the restatement of graphnorm.py:36-46 (scatter_mean = index_add / max(count, 1)) is segment_batches.ref_graphnorm
def make_case(D, sizes, scale=1.0, offset=0.0, shuffled=True, eps=1e-10):
    g = torch.Generator().manual_seed(2000 + D * 13 + sum(sizes) + len(sizes))
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffled:
        idx = idx[torch.randperm(idx.shape[0], generator=g)]
    x = torch.randn(idx.shape[0], D, generator=g) * scale + offset
    gout = torch.randn(idx.shape[0], D, generator=g)
    layer = L.GraphNorm(D, eps=eps)
    with torch.no_grad():
        layer.gamma.copy_(0.5 + torch.rand(1, D, generator=g))
        layer.alpha.copy_(0.5 + torch.rand(1, D, generator=g))
        layer.bias.copy_(torch.randn(1, D, generator=g))
    return layer.to(DEV), x.to(DEV), idx.to(DEV), gout.to(DEV)


def check_against_float64(D, sizes, scale=1.0, offset=0.0, shuffled=True, fused=True):
    layer, x, idx, gout = make_case(D, sizes, scale, offset, shuffled)
    before = ops.launch_counts(aggregation=True)
    got = run_layer(layer, x, idx, gout)
    ran = ops.launches_since(before)
    if fused:
        assert ran.get("graph_norm", 0) == 1 and ran.get("graph_norm_backward", 0) == 1, ran
    else:
        assert "graph_norm" not in ran and "graph_norm_backward" not in ran, ran
    res = {}
    for dt in (torch.float32, torch.float64):
        xr = x.detach().to(dt).clone().requires_grad_(True)
        p = [getattr(layer, k).detach().to(dt).clone().requires_grad_(True) for k in PARAMS]
        yr = ref_graphnorm(xr, idx, *p, 1e-10)
        yr.backward(gout.to(dt))
        res[dt] = {"y": yr.detach(), "x": xr.grad, "gamma": p[0].grad, "alpha": p[1].grad, "bias": p[2].grad}
    assert got["y"].shape == x.shape and got["y"].dtype == torch.float32
    for k, v in got.items():
        assert ok(v, res[torch.float32][k], res[torch.float64][k], k), k


# (D, nodes per graph, scale of x, offset of x)
SHAPES = [(64, [150, 1, 0, 57, 2, 300], 1.5, 0.0),
          (256, [2000, 1, 0, 300, 700, 128], 1.0, 0.0),
          (64, [50_000, 3, 0, 700], 1.0, 0.0),
          (64, [400, 2, 0, 90, 250], 0.01, 100.0),            # the mean dwarfs the spread
          (6, [300, 1, 0, 57, 129, 4], 1.0, 0.0),
          (64, [29_000] * 4, 1.0, 0.0),                        # the Graph2Class scale
          (512, [700, 1, 0, 129], 1.0, 0.0),
          (1024, [300, 1, 0, 2, 129], 1.0, 0.0),
          (100, [300, 1, 0, 2, 129], 1.0, 0.0)]                # a width that is not a multiple of 32


def shape_id(s):
    return f"D{s[0]}_n{sum(s[1])}_g{len(s[1])}" + (f"_x{s[2]:g}+{s[3]:g}" if (s[2], s[3]) != (1.0, 0.0) else "")


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_float64_restatement(shape, shuffled):
    D, sizes, scale, offset = shape
    check_against_float64(D, sizes, scale, offset, shuffled)


@pytest.mark.parametrize("rows", [127, 128, 129, 255, 256, 257])
def test_chunk_boundaries(rows):
    check_against_float64(64, [rows], shuffled=False)
    check_against_float64(6, [rows], shuffled=True)


def test_width_beyond_the_fused_kernels_takes_the_composed_route():
    assert ops.graph_norm_supported(1024) and not ops.graph_norm_supported(1100)
    check_against_float64(1100, [300, 1, 0, 2, 129], fused=False)
    layer, x, idx, _ = make_case(1100, [300, 1, 0, 2, 129])
    before = ops.launch_counts(aggregation=True)
    with torch.no_grad():
        layer(x, [], idx, {}, {}, [])
    ran = ops.launches_since(before)
    assert "graph_norm" not in ran and ran.get("k_gather_reduce", 0) >= 2, ran     # the facade's HIP scatter_mean


def test_two_runs_give_the_same_bits():
    layer, x, idx, gout = make_case(256, [3000, 1, 0, 500, 129, 77])
    a, b = run_layer(layer, x, idx, gout), run_layer(layer, x, idx, gout)
    assert set(a) == {"y", "x", "gamma", "alpha", "bias"}
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("D", [64, 100])
def test_a_graph_normalises_to_the_same_bits_alone_and_inside_a_batch(D):
    layer, x, idx, gout = make_case(D, [200, 57, 300, 40])
    rows = torch.nonzero(idx == 2).flatten()                      # the third graph, in the order its rows appear
    with torch.no_grad():
        whole = layer(x, [], idx, {}, {}, [])
        alone = layer(x[rows].contiguous(), [], torch.zeros(rows.shape[0], dtype=torch.int64, device=DEV), {}, {}, [])
    assert torch.equal(whole[rows], alone)
    batch = run_layer(layer, x, idx, gout)
    single = run_layer(layer, x[rows].contiguous(), torch.zeros(rows.shape[0], dtype=torch.int64, device=DEV),
                       gout[rows].contiguous())
    assert torch.equal(batch["y"][rows], single["y"]) and torch.equal(batch["x"][rows], single["x"])


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.ops.append((func.overloadpacket.__name__, [tuple(t.shape) for t in outs if isinstance(t, torch.Tensor)]))
        return out


def test_inference_writes_no_per_node_intermediate():
    N, D = 20_000, 64
    layer, x, idx, _ = make_case(D, [N // 4] * 4, shuffled=False)
    with torch.no_grad():
        layer(x, [], idx, {}, {}, [])                             # plan and graph count warmed
        before = ops.launch_counts(aggregation=True)
        with _Recorder() as rec:
            y = layer(x, [], idx, {}, {}, [])
        ran = ops.launches_since(before)
    assert ran == {"graph_norm": 1}, ran
    big = [(name, s) for name, s in rec.ops if (N, D) in s]
    assert [name for name, _ in big] == ["empty"], rec.ops         # the allocation of y and nothing else
    assert y.shape == (N, D)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_keep_their_dtype_and_equal_the_fp32_route(dtype):
    layer, x, idx, gout = make_case(64, [300, 1, 0, 57, 129])
    xh = x.to(dtype)
    before = ops.launch_counts(aggregation=True)
    with torch.no_grad():
        y = layer(xh, [], idx, {}, {}, [])
        y32 = layer(xh.float(), [], idx, {}, {}, [])
    assert ops.launches_since(before) == {"graph_norm": 2}
    assert y.dtype == dtype and y32.dtype == torch.float32
    assert torch.equal(y, y32.to(dtype))
    xr = xh.clone().requires_grad_(True)                          # training: the gradient comes back in the input's dtype
    layer(xr, [], idx, {}, {}, []).backward(gout.to(dtype))
    assert xr.grad.dtype == dtype and bool(torch.isfinite(xr.grad).all())


class _Embed(nn.Module):
    def forward(self, x):
        return x


def test_ggnn_graphnorm_ggnn_stack_eval_and_training_step_match_the_cpu_route():
    H, T = 64, 2
    torch.manual_seed(7)
    net = G.GraphNeuralNetwork([L.GatedMessagePassingLayer(H, H, 2 * T + 1, "sum"), L.GraphNorm(H, eps=1e-5),
                                L.GatedMessagePassingLayer(H, H, 2 * T + 1, "max")], _Embed(),
                               introduce_backwards_edges=True, add_self_edges=True)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        norm = net.message_passing_layers[1]
        norm.gamma.copy_(0.5 + torch.rand(1, H, generator=g))
        norm.alpha.copy_(0.5 + torch.rand(1, H, generator=g))
        norm.bias.copy_(torch.randn(1, H, generator=g) * 0.1)
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

    def call(module, dev, dt, train):
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
        ctx = torch.enable_grad() if train else torch.no_grad()
        with ctx:
            before = ops.launch_counts(aggregation=True)
            got = call(gpu, DEV, torch.float32, train)
            ran = ops.launches_since(before)
            want = {dt: call(m, "cpu", dt, train) for dt, m in cpu.items()}
        assert ran.get("graph_norm") == 1 and ran.get("graph_norm_backward", 0) == (1 if train else 0), ran
        assert set(got) == set(want[torch.float64])
        for k, v in got.items():
            assert ok(v, want[torch.float32][k], want[torch.float64][k], f"train={train} {k}"), (train, k)
