"""EGCMessagePassingLayer on the MI355X: reference fixtures (forward + gradients), both message forms on the fused
aggregate + combine kernel (and nothing on torch for the combine), a hub-sized graph against float64, per-edge dropout
in training, the combine backward at several shapes, AMP dtypes and the GNN container."""
import glob
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from helpers import dropout_keep_scale, to_cuda_adj
from oracle.fixtures import unpack_adj

pytestmark = pytest.mark.gpu

TOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYER_FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLDEN, "egc_*.npz")) if not f.endswith("egc_stack.npz"))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def prefixed(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}


def fixture_layer(fx):
    from ptgnn_amd.layers import EGCMessagePassingLayer
    H, D, T, K, B, _ = (int(v) for v in fx["meta"])
    layer = EGCMessagePassingLayer(H, D, T, str(fx["agg"]), num_bases=B, num_heads=K)
    layer.load_state_dict(prefixed(fx, "state."), strict=True)
    return layer


def call(layer, x, adj):
    feats = [torch.empty(s.shape[0], 0, device=x.device) for s, _ in adj]
    return layer(x, adj, None, {}, {}, feats)


def ref_egc(x, adj, layer, K, B, agg, mask=None):
    """egcmessagepassing.py:63-91 restated in torch (dtype of x, any device); `mask` scales the gathered rows."""
    sd = {k: v.to(x.dtype) for k, v in layer.state_dict().items()}
    T, N = len(adj), x.shape[0]
    w = x @ sd["_EGCMessagePassingLayer__weight_coeffs.weight"].t() + sd["_EGCMessagePassingLayer__weight_coeffs.bias"]
    inp = torch.cat([x[s] for s, _ in adj])
    if mask is not None:
        inp = inp * mask
    off = np.cumsum([0] + [int(s.shape[0]) for s, _ in adj])
    msgs = torch.cat([inp[off[t]:off[t + 1]] @ sd[f"_EGCMessagePassingLayer__bases.{t}.weight"].t() for t in range(T)])
    dst = torch.cat([d for _, d in adj])
    M = msgs.shape[1]
    out = torch.zeros(N, M, dtype=x.dtype, device=x.device)
    idx = dst.unsqueeze(1).expand(-1, M)
    if agg in ("sum", "mean"):
        out.scatter_add_(0, idx, msgs)
        if agg == "mean":
            cnt = torch.zeros(N, dtype=x.dtype, device=x.device).index_add_(0, dst, torch.ones_like(dst, dtype=x.dtype))
            out = out / cnt.clamp(min=1).unsqueeze(1)
    else:
        out.scatter_reduce_(0, idx, msgs, "amax" if agg == "max" else "amin", include_self=False)
    D = M // B
    return (out.view(N, K, B, D // K) * w.view(N, K, B, 1)).sum(2).reshape(N, D)


@pytest.fixture
def no_torch_linear(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("torch.nn.functional.linear was called on the EGC path")
    monkeypatch.setattr(torch.nn.functional, "linear", fail)


@pytest.mark.parametrize("path", LAYER_FIXTURES, ids=os.path.basename)
def test_fixture_forward_and_gradients_on_cuda(path, no_torch_linear):
    fx = load(path)
    layer = fixture_layer(fx).cuda()
    adj = to_cuda_adj(unpack_adj(fx))
    x = torch.from_numpy(fx["x"]).cuda()
    with torch.no_grad():
        y = call(layer.eval(), x, adj)
    np.testing.assert_allclose(y.cpu().numpy(), fx["y"], rtol=0, atol=TOL)
    layer.train()
    xg = x.clone().requires_grad_(True)
    y = call(layer, xg, adj)
    np.testing.assert_allclose(y.detach().cpu().numpy(), fx["y"], rtol=0, atol=TOL)
    (y * torch.from_numpy(fx["gout"]).cuda()).sum().backward()
    sc = max(1.0, float(np.abs(fx["grad.x"]).max()))
    np.testing.assert_allclose(xg.grad.cpu().numpy(), fx["grad.x"], rtol=0, atol=TOL * sc)
    for k, p in layer.named_parameters():
        want = fx["grad." + k]
        sc = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), want, rtol=0, atol=2 * TOL * sc, err_msg=k)


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        shapes = [tuple(a.shape) for a in args if isinstance(a, torch.Tensor)]
        self.ops.append((func.overloadpacket.__name__, shapes))
        return func(*args, **(kwargs or {}))


def sparse_types_graph(N, T, E, seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.multinomial(torch.ones(T), E, replacement=True, generator=g).bincount(minlength=T)
    return [(torch.randint(0, N, (int(c),), generator=g), torch.randint(0, N, (int(c),), generator=g)) for c in counts]


@pytest.mark.parametrize("form", ["table", "edge"])
@pytest.mark.parametrize("agg", ["sum", "max"])
def test_fused_inference_runs_one_combine_launch_and_no_torch_math(form, agg, no_torch_linear):
    from ptgnn_amd import layers as L, ops
    if form == "table":
        N, T, E = 2000, 3, 12000
    else:
        N, T, E = 3000, 12, 2500
    adj = sparse_types_graph(N, T, E, seed=3)
    H, D, K, B = 64, 128, 8, 4
    plan_sizes = (E, N, T, H, B * D)
    assert L._prefer_edge_path(*plan_sizes) == (form == "edge")
    torch.manual_seed(1)
    layer = L.EGCMessagePassingLayer(H, D, T, agg, num_bases=B, num_heads=K).cuda().eval()
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(2)).cuda()
    cadj = to_cuda_adj(adj)
    with torch.no_grad():
        call(layer, x, cadj)                      # plan built and cached outside the recorded call
        torch.cuda.synchronize()
        before = ops.launch_counts(aggregation=True)
        with _Recorder() as rec:
            y = call(layer, x, cadj)
        ran = ops.launches_since(before)
    assert ran.get("egc_gather_combine") == 1 and "k_gather_reduce" not in ran and "egc_combine" not in ran, ran
    on_rows = [(n, s) for n, s in rec.ops if n in ("mul", "sum") and any(len(t) > 0 and t[0] == N for t in s)]
    assert not on_rows, on_rows
    want = ref_egc(x.double(), [(s.cuda(), d.cuda()) for s, d in adj], layer, K, B, agg)
    assert float((y.double() - want).abs().max()) <= TOL


@pytest.mark.parametrize("agg", ["sum", "max"])
def test_large_graph_with_hub_row_against_float64(agg):
    from ptgnn_amd import layers as L, ops
    N, H, D, K, B, T = 20000, 128, 128, 8, 4, 3
    g = torch.Generator().manual_seed(7)
    adj = []
    for t in range(T):
        e = 48000
        s, d = torch.randint(0, N, (e,), generator=g), torch.randint(0, N, (e,), generator=g)
        if t == 0:   # one destination with 5000 in-edges: the hub path
            s = torch.cat([s, torch.randint(0, N, (5000,), generator=g)])
            d = torch.cat([d, torch.full((5000,), 11, dtype=torch.int64)])
        adj.append((s, d))
    torch.manual_seed(5)
    layer = L.EGCMessagePassingLayer(H, D, T, agg, num_bases=B, num_heads=K).cuda().eval()
    x = torch.randn(N, H, generator=g).cuda()
    cadj = to_cuda_adj(adj)
    ops.clear_plan_cache()
    plan = ops.plan_for(cadj, N)
    assert int(plan.hub_count.item()) > 0, "the 5000-edge row must take the hub path"
    with torch.no_grad():
        before = ops.launch_counts(aggregation=True)
        y = call(layer, x, cadj)
        ran = ops.launches_since(before)
        assert ran.get("egc_gather_combine") == 1, ran
        exact = ref_egc(x.double(), cadj, layer, K, B, agg)
        want32 = ref_egc(x, cadj, layer, K, B, agg)      # the reference's own fp32 arithmetic (torch on the GPU)
    err = float((y.double() - exact).abs().max())
    if agg == "max":
        assert err <= TOL
    else:  # benchmarks/common.py attributed_parity: strict, or no further from fp64 than 2x the fp32 reference is
        ref_err = float((want32.double() - exact).abs().max())
        assert float((y - want32).abs().max()) <= TOL or err <= max(TOL, 2.0 * ref_err), (err, ref_err)


@pytest.mark.parametrize("agg", ["sum", "max"])
def test_training_with_per_edge_dropout(agg, monkeypatch):
    from ptgnn_amd import layers as L
    N, T, E, H, D, K, B, p, seed = 400, 3, 1600, 32, 64, 8, 4, 0.1, 123456789123
    adj = sparse_types_graph(N, T, E, seed=9)
    torch.manual_seed(4)
    layer = L.EGCMessagePassingLayer(H, D, T, agg, num_bases=B, num_heads=K, dropout_rate=p).cuda().train()
    monkeypatch.setattr(L, "_dropout_seed", lambda: seed)
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(8)).cuda()
    cadj = to_cuda_adj(adj)
    xg = x.clone().requires_grad_(True)
    y = call(layer, xg, cadj)
    mask = dropout_keep_scale(seed, E, H, p).cuda().double()
    xo = x.double().requires_grad_(True)
    want = ref_egc(xo, cadj, layer, K, B, agg, mask=mask)
    assert float((y.double() - want).abs().max()) <= TOL
    gout = torch.randn(N, D, generator=torch.Generator().manual_seed(10)).cuda()
    y.backward(gout)
    want.backward(gout.double())
    sc = max(1.0, float(xo.grad.abs().max()))
    assert float((xg.grad.double() - xo.grad).abs().max()) <= 2 * TOL * sc


@pytest.mark.parametrize("K,B,Dh", [(8, 4, 16), (4, 2, 32), (3, 3, 12), (2, 3, 5)])
def test_combine_forward_and_backward_against_float64(K, B, Dh):
    from ptgnn_amd import dense, ops
    n = 1037
    g = torch.Generator().manual_seed(K * 100 + B * 10 + Dh)
    agg = torch.randn(n, K * B * Dh, generator=g).cuda()
    coef = torch.randn(n, K * B, generator=g).cuda()
    gout = torch.randn(n, K * Dh, generator=g).cuda()
    a64, c64 = agg.double().requires_grad_(True), coef.double().requires_grad_(True)
    want = (a64.view(n, K, B, Dh) * c64.view(n, K, B, 1)).sum(2).reshape(n, K * Dh)
    want.backward(gout.double())
    before = ops.launch_counts(aggregation=True)
    ag, cg = agg.clone().requires_grad_(True), coef.clone().requires_grad_(True)
    y = dense.basis_combine(ag, cg, K, B, Dh)
    y.backward(gout)
    ran = ops.launches_since(before)
    assert ran == {"egc_combine": 1, "egc_combine_backward": 1}, ran
    assert float((y.double() - want).abs().max()) <= TOL
    assert float((ag.grad.double() - a64.grad).abs().max()) <= TOL
    assert float((cg.grad.double() - c64.grad).abs().max()) <= TOL * max(1.0, float(c64.grad.abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_amp_dtype_in_same_dtype_out(dtype):
    from ptgnn_amd import layers as L
    N, T = 500, 3
    adj = to_cuda_adj(sparse_types_graph(N, T, 2000, seed=12))
    torch.manual_seed(6)
    layer = L.EGCMessagePassingLayer(32, 64, T, "mean", num_bases=4, num_heads=8).cuda().eval()
    x = torch.randn(N, 32, generator=torch.Generator().manual_seed(13)).cuda().to(dtype)
    with torch.no_grad():
        y = call(layer, x, adj)
        y32 = call(layer, x.float(), adj)
    assert y.dtype == dtype
    assert torch.equal(y, y32.to(dtype))


def test_gnn_container_cuda_equals_cpu_and_reference():
    from ptgnn_amd.gnn import GraphNeuralNetwork
    from ptgnn_amd.layers import EGCMessagePassingLayer, MeanResidualLayer
    fx = load(os.path.join(GOLDEN, "egc_stack.npz"))
    x = torch.from_numpy(fx["x"])
    H = x.shape[1]
    T = 2 * int(fx["__num_edge_types__"]) + 1
    e0 = EGCMessagePassingLayer(H, H, T, "sum", num_bases=4, num_heads=8)
    e1 = EGCMessagePassingLayer(H, H, T, "max", num_bases=2, num_heads=4)
    e0.load_state_dict(prefixed(fx, "l0."), strict=True)
    e1.load_state_dict(prefixed(fx, "l1."), strict=True)
    r = MeanResidualLayer(H)
    net = GraphNeuralNetwork([r.pass_through_dummy_layer(), e0, e1, r], torch.nn.Identity(),
                             introduce_backwards_edges=True, add_self_edges=True).eval()
    adj, ntg = unpack_adj(fx), torch.from_numpy(fx["node_to_graph_idx"])

    def run(dev):
        with torch.no_grad():
            return net.to(dev)(node_data={"input": x.to(dev)}, adjacency_lists=[(s.to(dev), d.to(dev)) for s, d in adj],
                               edge_feature_data=[], node_to_graph_idx=ntg.to(dev), reference_node_ids={},
                               reference_node_graph_idx={}, num_graphs=3).output_node_representations.cpu()
    cpu = run("cpu")
    gpu = run("cuda")
    assert float((gpu - cpu).abs().max()) <= TOL
    assert float((gpu - torch.from_numpy(fx["y"])).abs().max()) <= TOL
