"""PnaMessageAggregation on the MI355X, alone and inside MlpMessagePassingLayer: reference fixtures (forward + gradients),
both message forms on ONE fused launch with GELU + LayerNorm inside (no torch op on an [N, 15M] tensor), a ~50 k-in-edge
hub row against float64 and run-to-run bits, tie routing, empty rows, widths 6 and 256, unsorted standalone targets,
half / bfloat16 dtype semantics and a training step against a float64 autograd restatement.

Error bar (benchmarks/common.py attributed_parity): strict 1e-5, or -- where the std block's cancellation makes fp32
itself miss that -- no further from float64 than max(1e-5, 2x the fp32 reference's own distance from float64)."""
import copy
import glob
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from agg_paths import TOL, attributed_ok, pna_ref
from helpers import to_cuda_adj
from oracle.fixtures import unpack_adj

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYER_FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLDEN, "pna_*.npz"))
                        if not f.endswith(("pna_stack.npz", "pna_module.npz")))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def prefixed(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}


class Pna64(torch.nn.Module):
    def __init__(self, delta):
        super().__init__()
        self.delta = delta

    def forward(self, messages, message_targets, num_nodes):
        return pna_ref(messages, message_targets, int(num_nodes), self.delta)


def restated(layer, dtype):
    """The layer on the CPU in `dtype` with the aggregation restated in that dtype (float64: the exact reference)."""
    from ptgnn_amd.layers import PnaMessageAggregation
    ref = copy.deepcopy(layer).cpu().to(dtype)
    agg = ref._MlpMessagePassingLayer__aggregation_fn
    assert isinstance(agg, PnaMessageAggregation)
    ref._MlpMessagePassingLayer__aggregation_fn = Pna64(agg._delta)
    return ref


def call(layer, x, adj):
    feats = [torch.empty(s.shape[0], 0, device=x.device) for s, _ in adj]
    return layer(x, adj, None, {}, {}, feats)


def fixture_layer(fx):
    from ptgnn_amd.layers import MlpMessagePassingLayer, PnaMessageAggregation
    H, M, D, T, hidden, target, ln, dense, _ = (int(v) for v in fx["meta"])
    layer = MlpMessagePassingLayer(H, D, M, T, PnaMessageAggregation(delta=float(fx["delta"])),
                                   use_target_state_as_message_input=bool(target), mlp_hidden_layers=hidden,
                                   use_layer_norm=bool(ln), use_dense_layer=bool(dense))
    layer.load_state_dict(prefixed(fx, "state."), strict=True)
    return layer


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", LAYER_FIXTURES, ids=os.path.basename)
def test_fixture_forward_and_gradients_on_cuda(path):
    fx = load(path)
    layer = fixture_layer(fx)
    adj_cpu = unpack_adj(fx)
    x_cpu = torch.from_numpy(fx["x"])
    # float64 attribution of the fixture's own fp32 values
    ref = restated(layer, torch.float64)
    x64 = x_cpu.double().requires_grad_(True)
    y64 = call(ref, x64, adj_cpu)
    (y64 * torch.from_numpy(fx["gout"]).double()).sum().backward()

    layer = layer.cuda()
    adj = to_cuda_adj(adj_cpu)
    x = x_cpu.cuda()
    with torch.no_grad():
        y = call(layer.eval(), x, adj)
    assert attributed_ok(y, fx["y"], y64), float((y.cpu() - torch.from_numpy(fx["y"])).abs().max())
    layer.train()
    xg = x.clone().requires_grad_(True)
    y = call(layer, xg, adj)
    assert attributed_ok(y, fx["y"], y64)
    (y * torch.from_numpy(fx["gout"]).cuda()).sum().backward()
    sc = max(1.0, float(np.abs(fx["grad.x"]).max()))
    assert attributed_ok(xg.grad, fx["grad.x"], x64.grad, scale=sc), "grad.x"
    p64 = dict(ref.named_parameters())
    for k, p in layer.named_parameters():
        want = fx["grad." + k]
        sc = max(1.0, float(np.abs(want).max()))
        assert attributed_ok(p.grad, want, p64[k].grad, tol=2 * TOL, scale=sc), k


def test_module_fixture_unsorted_targets_on_cuda():
    from ptgnn_amd.layers import PnaMessageAggregation
    fx = load(os.path.join(GOLDEN, "pna_module.npz"))
    t_cpu = torch.from_numpy(fx["targets"])
    n = int(fx["num_nodes"])
    assert n > int(t_cpu.max()) + 1 and not bool((t_cpu[1:] >= t_cpu[:-1]).all())
    m64 = torch.from_numpy(fx["messages"]).double().requires_grad_(True)
    out64 = pna_ref(m64, t_cpu, n, 1.0)
    (out64 * torch.from_numpy(fx["gout"]).double()).sum().backward()
    m = torch.from_numpy(fx["messages"]).cuda().requires_grad_(True)
    out = PnaMessageAggregation(delta=float(fx["delta"]))(messages=m, message_targets=t_cpu.cuda(), num_nodes=n)
    assert out.dtype == torch.float32 and out.shape == (n, 15 * m.shape[1])
    assert attributed_ok(out, fx["out"], out64)
    (out * torch.from_numpy(fx["gout"]).cuda()).sum().backward()
    sc = max(1.0, float(np.abs(fx["grad"]).max()))
    assert attributed_ok(m.grad, fx["grad"], m64.grad, scale=sc)


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


@pytest.mark.parametrize("form,M", [("table", 32), ("edge", 32), ("table", 256), ("table1", 32), ("table1", 6)])
def test_fused_inference_runs_one_pna_launch_and_no_wide_torch_op(form, M):
    """table1: one edge type, so the destination term is one row per destination (the DST == 2 kernel variant)."""
    from ptgnn_amd import layers as L, ops
    if form == "table":
        N, T, E = 2000, 3, 12000
    elif form == "table1":
        N, T, E = 2000, 1, 6000
    else:
        N, T, E = 3000, 12, 2500
    H = 64
    adj = sparse_types_graph(N, T, E, seed=3)
    assert L._prefer_edge_path(E, N, T, H, M) == (form == "edge")
    torch.manual_seed(1)
    layer = L.MlpMessagePassingLayer(H, 48, M, T, L.PnaMessageAggregation(delta=1.5)).cuda().eval()
    x = torch.randn(N, H, generator=torch.Generator().manual_seed(2)).cuda()
    cadj = to_cuda_adj(adj)
    with torch.no_grad():
        call(layer, x, cadj)                      # plan built and cached outside the recorded call
        torch.cuda.synchronize()
        before = ops.launch_counts(aggregation=True)
        with _Recorder() as rec:
            y = call(layer, x, cadj)
        ran = ops.launches_since(before)
    assert ran.get("pna_aggregate") == 1 and "k_gather_reduce" not in ran, ran
    wide = [(n, s) for n, s in rec.ops if any(len(t) == 2 and t[1] == 15 * M for t in s)]
    assert not wide, wide
    want32 = call(restated(layer, torch.float32), x.cpu(), adj)
    exact = call(restated(layer, torch.float64), x.cpu().double(), adj)
    assert attributed_ok(y, want32, exact)


@pytest.mark.parametrize("M", [6, 64])
def test_hub_row_against_float64_and_bitwise_repeatable(M):
    from ptgnn_amd import ops
    from ptgnn_amd.layers import PnaMessageAggregation
    g = torch.Generator().manual_seed(11)
    N, E_rest, HUB = 20000, 60000, 50000
    t = torch.cat([torch.randint(0, N, (E_rest,), generator=g), torch.full((HUB,), 17, dtype=torch.int64)])
    t = t[torch.randperm(t.shape[0], generator=g)]
    m_cpu = torch.randn(t.shape[0], M, generator=g)
    gout = torch.randn(N, 15 * M, generator=g)
    agg = PnaMessageAggregation()
    m = m_cpu.cuda().requires_grad_(True)
    before = ops.launch_counts(aggregation=True)
    out = agg(messages=m, message_targets=t.cuda(), num_nodes=N)
    assert ops.launches_since(before).get("pna_aggregate") == 1
    with torch.no_grad():
        again = agg(messages=m.detach(), message_targets=t.cuda(), num_nodes=N)
    assert torch.equal(out.detach(), again), "two calls differ"
    (out * gout.cuda()).sum().backward()
    m64 = m_cpu.double().requires_grad_(True)
    out64 = pna_ref(m64, t, N, 1.0)
    (out64 * gout.double()).sum().backward()
    m32 = m_cpu.clone().requires_grad_(True)
    out32 = pna_ref(m32, t, N, 1.0)
    (out32 * gout).sum().backward()
    assert attributed_ok(out, out32, out64)
    sc = max(1.0, float(m64.grad.abs().max()))
    assert attributed_ok(m.grad, m32.grad, m64.grad, scale=sc)


def test_ties_route_the_gradient_to_the_earliest_slot():
    from ptgnn_amd.layers import PnaMessageAggregation
    M = 8
    row = torch.randn(1, M, generator=torch.Generator().manual_seed(5))
    m = torch.cat([torch.randn(3, M), row, row, torch.randn(2, M), row]).cuda().requires_grad_(True)
    t = torch.tensor([1, 2, 1, 0, 0, 2, 1, 0]).cuda()       # node 0 gets rows 3, 4, 7: all equal
    out = PnaMessageAggregation()(messages=m, message_targets=t, num_nodes=3)
    for blk in (2, 3):                                       # max, min
        if m.grad is not None:
            m.grad = None
        sel = torch.zeros_like(out)
        sel[0, blk * M:(blk + 1) * M] = 1.0
        (out * sel).sum().backward(retain_graph=True)
        gr = m.grad.cpu()
        assert torch.equal(gr[3], torch.ones(M)) and float(gr[4].abs().max()) == 0 and float(gr[7].abs().max()) == 0


def test_empty_rows_are_zero_with_finite_gradients():
    from ptgnn_amd.layers import PnaMessageAggregation
    g = torch.Generator().manual_seed(6)
    t = torch.tensor([0, 0, 2, 5, 5, 5])                     # rows 1, 3, 4, 6, 7 are empty
    m = torch.randn(6, 4, generator=g).cuda().requires_grad_(True)
    out = PnaMessageAggregation(delta=2.5)(messages=m, message_targets=t.cuda(), num_nodes=8)
    for r in (1, 3, 4, 6, 7):
        assert float(out[r].abs().max()) == 0.0
    out.sum().backward()
    assert bool(torch.isfinite(m.grad).all())


@pytest.mark.parametrize("M", [6, 256])
def test_widths_against_float64(M):
    from ptgnn_amd.layers import PnaMessageAggregation
    g = torch.Generator().manual_seed(M)
    N, E = 3000, 9000
    t = torch.randint(0, N, (E,), generator=g)
    m_cpu = torch.randn(E, M, generator=g)
    gout = torch.randn(N, 15 * M, generator=g)
    m = m_cpu.cuda().requires_grad_(True)
    out = PnaMessageAggregation()(messages=m, message_targets=t.cuda(), num_nodes=N)
    (out * gout.cuda()).sum().backward()
    m64, m32 = m_cpu.double().requires_grad_(True), m_cpu.clone().requires_grad_(True)
    out64, out32 = pna_ref(m64, t, N, 1.0), pna_ref(m32, t, N, 1.0)
    (out64 * gout.double()).sum().backward()
    (out32 * gout).sum().backward()
    assert attributed_ok(out, out32, out64)
    assert attributed_ok(m.grad, m32.grad, m64.grad, scale=max(1.0, float(m64.grad.abs().max())))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_messages_round_the_aggregate_and_promote(dtype):
    from ptgnn_amd import torch_route
    from ptgnn_amd.layers import PnaMessageAggregation
    g = torch.Generator().manual_seed(9)
    N, E, M = 500, 2000, 16
    t = torch.randint(0, N, (E,), generator=g)
    m = torch.randn(E, M, generator=g).to(dtype)
    out = PnaMessageAggregation()(messages=m.cuda(), message_targets=t.cuda(), num_nodes=N)
    assert out.dtype == torch.float32
    assert torch.equal(out[:, :5 * M].cpu(), out[:, :5 * M].cpu().to(dtype).float())   # block A: message-dtype values
    want = torch_route.pna_aggregate(m, t, N, 1)
    assert want.dtype == torch.float32
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=ulp, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_messages_gradient_matches_reference_autograd(dtype):
    """The reference rounds A to the message dtype and backpropagates through the UNROUNDED fp32 mean / std; its block
    gradients are message-dtype tensors.  Bar: one unit in the last place of the message dtype, times 4, of the largest
    gradient (fp32 reorderings in the std terms stay far below it)."""
    from ptgnn_amd import torch_route
    from ptgnn_amd.layers import PnaMessageAggregation
    g = torch.Generator().manual_seed(13)
    N, E, M = 400, 900, 8                                   # in-degree ~2: many degree-1 and degree-2 rows
    t = torch.randint(0, N, (E,), generator=g)
    m = torch.randn(E, M, generator=g).to(dtype)
    gout = torch.randn(N, 15 * M, generator=g)
    mr = m.clone().requires_grad_(True)
    want = torch_route.pna_aggregate(mr, t, N, 1)           # the reference's operators on the CPU
    (want * gout).sum().backward()
    mg = m.cuda().requires_grad_(True)
    out = PnaMessageAggregation()(messages=mg, message_targets=t.cuda(), num_nodes=N)
    (out * gout.cuda()).sum().backward()
    assert mg.grad.dtype == dtype and mr.grad.dtype == dtype
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    ref = mr.grad.float()
    err = float((mg.grad.float().cpu() - ref).abs().max())
    assert bool(torch.isfinite(mg.grad.float()).all())
    assert err <= 4 * ulp * max(1.0, float(ref.abs().max())), (err, float(ref.abs().max()))


def test_training_step_against_float64_autograd():
    from ptgnn_amd import layers as L
    g = torch.Generator().manual_seed(21)
    N, T, H, M, D = 20000, 2, 32, 32, 32
    adj = [(torch.randint(0, N, (40000,), generator=g), torch.randint(0, N, (40000,), generator=g)) for _ in range(T)]
    torch.manual_seed(3)
    layer = L.MlpMessagePassingLayer(H, D, M, T, L.PnaMessageAggregation()).cuda().train()
    x_cpu = torch.randn(N, H, generator=g)
    gout = torch.randn(N, D, generator=g)
    ref64, ref32 = restated(layer, torch.float64), restated(layer, torch.float32)
    x64, x32 = x_cpu.double().requires_grad_(True), x_cpu.clone().requires_grad_(True)
    y64, y32 = call(ref64, x64, adj), call(ref32, x32, adj)
    (y64 * gout.double()).sum().backward()
    (y32 * gout).sum().backward()
    xg = x_cpu.cuda().requires_grad_(True)
    y = call(layer, xg, to_cuda_adj(adj))
    (y * gout.cuda()).sum().backward()
    assert attributed_ok(y, y32, y64)
    assert attributed_ok(xg.grad, x32.grad, x64.grad, scale=max(1.0, float(x64.grad.abs().max())))
    p64, p32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    for k, p in layer.named_parameters():
        sc = max(1.0, float(p64[k].grad.abs().max()))
        assert attributed_ok(p.grad, p32[k].grad, p64[k].grad, tol=2 * TOL, scale=sc), k


def test_subclass_keeps_the_general_path():
    from ptgnn_amd import layers as L, ops

    class MyPna(L.PnaMessageAggregation):
        pass
    N, T, H, M = 300, 2, 32, 8
    adj = to_cuda_adj(sparse_types_graph(N, T, 900, seed=4))
    torch.manual_seed(2)
    layer = L.MlpMessagePassingLayer(H, 16, M, T, MyPna()).cuda().eval()
    x = torch.randn(N, H).cuda()
    with torch.no_grad():
        before = ops.launch_counts(aggregation=True)
        y = call(layer, x, adj)
        ran = ops.launches_since(before)
    assert ran.get("pna_aggregate") == 1                   # the module's own launch, over its own plan
    exact = call(restated(layer, torch.float64), x.cpu().double(), [(s.cpu(), d.cpu()) for s, d in adj])
    want32 = call(restated(layer, torch.float32), x.cpu(), [(s.cpu(), d.cpu()) for s, d in adj])
    assert attributed_ok(y, want32, exact)


def test_gnn_container_cuda_equals_reference():
    from ptgnn_amd.gnn import GraphNeuralNetwork
    from ptgnn_amd.layers import MeanResidualLayer, MlpMessagePassingLayer, PnaMessageAggregation
    fx = load(os.path.join(GOLDEN, "pna_stack.npz"))
    x = torch.from_numpy(fx["x"])
    H = x.shape[1]
    T = 2 * int(fx["__num_edge_types__"]) + 1
    l0 = MlpMessagePassingLayer(H, H, 8, T, PnaMessageAggregation())
    l1 = MlpMessagePassingLayer(H, H, 32, T, PnaMessageAggregation(delta=2.0), use_target_state_as_message_input=False)
    l0.load_state_dict(prefixed(fx, "l0."), strict=True)
    l1.load_state_dict(prefixed(fx, "l1."), strict=True)
    r = MeanResidualLayer(H)
    net = GraphNeuralNetwork([r.pass_through_dummy_layer(), l0, l1, r], torch.nn.Identity(),
                             introduce_backwards_edges=True, add_self_edges=True).cuda().eval()
    with torch.no_grad():
        out = net(node_data={"input": x.cuda()}, adjacency_lists=to_cuda_adj(unpack_adj(fx)), edge_feature_data=[],
                  node_to_graph_idx=torch.from_numpy(fx["node_to_graph_idx"]).cuda(), reference_node_ids={},
                  reference_node_graph_idx={}, num_graphs=3)
    np.testing.assert_allclose(out.output_node_representations.cpu().numpy(), fx["y"], rtol=0, atol=2 * TOL)
