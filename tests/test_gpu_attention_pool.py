"""The attention reducers on the MI355X: the fused HIP segment-softmax pool (csrc/attention_pool.hip) against the
reference fixtures, a float64 restatement of the reference's operator order at D in {4, 6, 64, 256, 512} and the
Graph2Seq shape, determinism, the no-[N, heads * D] guarantee, AMP dtypes and the global exchange around it -- and, with
the weighted-sum pool (csrc/weighted_pool.hip), the chunk rule the two pools share (csrc/segment_chunks.h): the 128-row
chunk boundaries, and a sample pooling to the same bits alone and inside a batch."""
import copy
import math
import types

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from agg_paths import TOL, attributed_ok
from attnpool_cases import CASES, NUM_SAMPLES, build
from ptgnn_amd import _lib, ops, reduceops as R
from segment_batches import ref_multihead, ref_weighted

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXTURE_TOL = 2e-5


def load(name):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    return {k: z[k] for k in z.files}


def rel_err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().double().cpu() - want.cpu()).abs().max()) / max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    fx = load(name)
    module = build(spec, R)
    module.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}, strict=True)
    module = module.to(DEV)
    x = torch.from_numpy(fx["x"]).to(DEV).requires_grad_(True)
    before = ops.launch_counts(aggregation=True)
    y = module(R.ElementsToSummaryRepresentationInput(x, torch.from_numpy(fx["index"]).to(DEV), NUM_SAMPLES))
    (y * torch.from_numpy(fx["gout"]).to(DEV)).sum().backward()
    ran = ops.launches_since(before)
    assert ran.get("attention_pool", 0) >= 1 and ran.get("attention_pool_backward", 0) >= 1, ran
    assert rel_err(y, fx["y"]) <= FIXTURE_TOL
    assert rel_err(x.grad, fx["grad.x"]) <= FIXTURE_TOL
    for k, p in module.named_parameters():
        assert rel_err(p.grad, fx["grad." + k]) <= FIXTURE_TOL, k


# the float64 restatement of varsizedsummary.py:140-178 with a `max` query (hidden = D) is segment_batches.ref_multihead

# (D, heads, value layer, sizes of the samples, scale of x); every shape ends with an empty sample
SHAPES = [(4, h, False, [300, 1, 0, 57, 129, 4], 1.0) for h in (1, 2, 4)]
SHAPES += [(6, h, v, [300, 1, 0, 57, 129, 4], 1.0) for h, v in ((1, False), (2, True), (3, False), (6, False))]
SHAPES += [(64, h, False, [300, 1, 0, 57, 129, 4], 1.0) for h in (1, 4, 8)]
SHAPES += [(64, 4, True, [50_000, 3, 0, 700], 1.0),                     # a 50 k-element sample
           (64, 8, False, [400, 2, 0, 90, 250], 8.0),                   # scores spanning far more than 100
           (64, 16, False, [300, 1, 0, 57, 129, 4], 1.0),               # 16 heads: beyond the fused range
           (256, 8, False, [2000, 1, 0, 300, 700, 128], 1.0),           # Graph2Seq: D = hidden = 256, 8 heads
           (256, 4, True, [900, 1, 0, 129], 1.0),
           (512, 4, False, [700, 1, 0, 129], 1.0),
           (512, 8, True, [700, 1, 0, 129], 1.0)]


def shape_id(s):
    return f"D{s[0]}_h{s[1]}{'_v' if s[2] else ''}_n{sum(s[3])}{'_x%g' % s[4] if s[4] != 1 else ''}"


def make_case(D, H, value, sizes, scale, seed=0):
    g = torch.Generator().manual_seed(1000 + D * 17 + H + sum(sizes))
    G = len(sizes) + 1
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    idx = idx[torch.randperm(idx.shape[0], generator=g)]
    x = torch.randn(idx.shape[0], D, generator=g) * scale
    torch.manual_seed(seed)
    module = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, 32, H, R.SimpleVarSizedElementReduce("max"),
                                                           use_value_layer=value)
    gout = torch.randn(G, 32, generator=g)
    return module, x, idx, G, gout


def weights(module, dtype):
    sd = {k.split("__")[-1]: v.to(DEV, dtype) for k, v in module.state_dict().items()}
    return sd["key_layer.weight"], sd.get("value_layer.weight"), sd["output_layer.weight"]


def check_against_float64(D, H, value, sizes, scale):
    module, x, idx, G, gout = make_case(D, H, value, sizes, scale)
    module = module.to(DEV)
    xd, idxd, goutd = x.to(DEV).requires_grad_(True), idx.to(DEV), gout.to(DEV)
    before = ops.launch_counts(aggregation=True)
    y = module(R.ElementsToSummaryRepresentationInput(xd, idxd, G))
    y.backward(goutd)
    ran = ops.launches_since(before)
    fused = ops.attention_pool_supported(D, H)
    assert fused == (H <= 8)
    assert (ran.get("attention_pool", 0) == 1 and ran.get("attention_pool_backward", 0) == 1) == fused, ran
    got = {"y": y, "x": xd.grad}
    got.update({k.split("__")[-1]: p.grad for k, p in module.named_parameters()})
    res = {}
    for dt in (torch.float32, torch.float64):
        xr = x.detach().to(DEV, dt).clone().requires_grad_(True)
        w = [t.requires_grad_(True) if t is not None else None for t in weights(module, dt)]
        yr, scores = ref_multihead(xr, idxd, G, *w, H)
        yr.backward(goutd.to(dt))
        res[dt] = {"y": yr, "x": xr.grad, "key_layer.weight": w[0].grad, "output_layer.weight": w[2].grad}
        if value:
            res[dt]["value_layer.weight"] = w[1].grad
    if scale != 1.0:
        spans = [float(scores[idxd == s].max() - scores[idxd == s].min()) for s in range(len(sizes)) if sizes[s] > 1]
        assert max(spans) > 100.0                    # exp overflows without the running max
    for k, v in got.items():
        exact = res[torch.float64][k]
        assert attributed_ok(v, res[torch.float32][k], exact, TOL, max(1.0, float(exact.detach().abs().max()))), k
    return y


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_float64_restatement(shape):
    y, sizes = check_against_float64(*shape), shape[3]
    assert float(y[len(sizes)].abs().max()) == 0.0 and float(y[sizes.index(0)].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the chunk rule of csrc/segment_chunks.h under both pools
# ---------------------------------------------------------------------------------------------------------------------
def check_weighted_against_float64(D, sizes, shuffled):
    g = torch.Generator().manual_seed(3000 + D * 11 + sum(sizes))
    G = len(sizes)
    idx = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    if shuffled:
        idx = idx[torch.randperm(idx.shape[0], generator=g)]
    x, w = torch.randn(idx.shape[0], D, generator=g).to(DEV), (torch.randn(1, D, generator=g) / math.sqrt(D)).to(DEV)
    gout, idx = torch.randn(G, D, generator=g).to(DEV), idx.to(DEV)
    plan = ops.plan_for([(idx, idx)], G) if shuffled else ops.plan_from_sorted_index(idx, G)
    got = {"out": ops.weighted_pool(x, w, plan)}
    got["x"], got["w"] = ops.weighted_pool_backward(x, w, idx, gout)
    res = {}
    for dt in (torch.float32, torch.float64):
        xr, wr = x.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
        out = ref_weighted(xr, idx, G, wr)
        out.backward(gout.to(dt))
        res[dt] = {"out": out.detach(), "x": xr.grad, "w": wr.grad.reshape(-1)}
    for k, v in got.items():
        exact = res[torch.float64][k]
        print(f"weighted pool D={D} n={sum(sizes)} {k}: |got-fp32|={float((v - res[torch.float32][k]).abs().max()):.3e} "
              f"|got-f64|={float((v.double() - exact).abs().max()):.3e} scale={float(exact.abs().max()):.3e}")
        assert attributed_ok(v, res[torch.float32][k], exact, TOL, max(1.0, float(exact.abs().max()))), k


@pytest.mark.parametrize("rows", [127, 128, 129, 255, 256, 257])
def test_chunk_boundaries(rows):
    check_weighted_against_float64(64, [rows], shuffled=False)
    check_weighted_against_float64(6, [rows, 5], shuffled=True)      # a second sample, so that the shuffle moves rows
    check_against_float64(64, 4, False, [rows], 1.0)
    check_against_float64(6, 3, False, [rows], 1.0)


@pytest.mark.parametrize("D", [64, 100])
def test_a_sample_pools_to_the_same_bits_alone_and_inside_a_batch(D):
    """Chunks are counted from a sample's own start, so its pool and its gradients do not depend on the samples around
    it.  (Not the weighted pool's weight gradient: that folds 256-row blocks of the whole batch.)"""
    sizes, H = [200, 57, 300, 40], 4
    g = torch.Generator().manual_seed(4000 + D)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    x, w = torch.randn(idx.shape[0], D, generator=g).to(DEV), (torch.randn(1, D, generator=g) / math.sqrt(D)).to(DEV)
    u = (torch.randn(len(sizes), H, D, generator=g) / math.sqrt(D)).to(DEV)
    gout, gpool = torch.randn(len(sizes), D, generator=g).to(DEV), torch.randn(len(sizes), H, D, generator=g).to(DEV)
    rows = torch.nonzero(idx == 2).flatten()
    x1, idx1 = x[rows].contiguous(), torch.zeros(rows.shape[0], dtype=torch.int64, device=DEV)
    plan, plan1 = ops.plan_from_sorted_index(idx, len(sizes)), ops.plan_from_sorted_index(idx1, 1)

    assert torch.equal(ops.weighted_pool(x, w, plan)[2], ops.weighted_pool(x1, w, plan1)[0])
    gx, _ = ops.weighted_pool_backward(x, w, idx, gout)
    gx1, _ = ops.weighted_pool_backward(x1, w, idx1, gout[2:3].contiguous())
    assert torch.equal(gx[rows], gx1)

    pooled, stats = ops.attention_pool(x, u, plan)
    pooled1, stats1 = ops.attention_pool(x1, u[2:3].contiguous(), plan1)
    assert torch.equal(pooled[2], pooled1[0]) and torch.equal(stats[2], stats1[0])
    gx, gu = ops.attention_pool_backward(x, u, plan, pooled, stats, gpool)
    gx1, gu1 = ops.attention_pool_backward(x1, u[2:3].contiguous(), plan1, pooled1, stats1, gpool[2:3].contiguous())
    assert torch.equal(gx[rows], gx1) and torch.equal(gu[2], gu1[0])


def test_two_runs_give_the_same_bits():
    module, x, idx, G, gout = make_case(256, 8, True, [3000, 1, 0, 500, 129], 1.0)
    module = module.to(DEV)
    outs = []
    for _ in range(2):
        module.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        y = module(R.ElementsToSummaryRepresentationInput(xd, idx.to(DEV), G))
        y.backward(gout.to(DEV))
        outs.append([y.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in module.parameters()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_empty_samples_give_zero_output_and_zero_gradient():
    module, x, idx, G, gout = make_case(64, 4, True, [200, 0, 30], 1.0)
    module = module.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = module(R.ElementsToSummaryRepresentationInput(xd, idx.to(DEV), G))
    empty = [1, G - 1]
    assert float(y[empty].abs().max()) == 0.0
    only_empty = torch.zeros_like(y)
    only_empty[empty] = gout.to(DEV)[empty]
    y.backward(only_empty)
    assert float(xd.grad.abs().max()) == 0.0
    for p in module.parameters():
        assert float(p.grad.abs().max()) == 0.0


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.ops.append((func.overloadpacket.__name__, [tuple(t.shape) for t in outs if isinstance(t, torch.Tensor)]))
        return out


def test_graph2seq_inference_writes_no_per_element_head_tensor_and_calls_no_gemm():
    """graph2seq.py:116-122: D = hidden = 256, 8 heads, `max` query; the fused path from the reducer's forward on."""
    D, H, N = 256, 8, 20_000
    torch.manual_seed(3)
    module = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, 128, H, R.SimpleVarSizedElementReduce("max")).to(DEV)
    idx = torch.sort(torch.randint(0, 40, (N,), device=DEV)).values
    x = torch.randn(N, D, device=DEV)
    inp = R.ElementsToSummaryRepresentationInput(x, idx, 40)
    with torch.no_grad():
        module(inp)                                    # plan and query pool warmed
        before = ops.launch_counts(aggregation=True)
        with _Recorder() as rec:
            y = module(inp)
        ran = ops.launches_since(before)
    assert ran.get("attention_pool") == 1 and ran.get("head_projection") == 1, ran
    big = [(name, s) for name, s in rec.ops for t in s if t in ((N, H * D), (N, D), (N, H, D))]
    assert not big, big
    assert not {name for name, _ in rec.ops} & {"linear", "mm", "addmm", "bmm", "matmul"}, rec.ops
    assert y.shape == (40, 128)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_return_their_dtype(dtype):
    module, x, idx, G, _ = make_case(64, 4, False, [300, 1, 0, 57], 1.0)
    module = module.to(DEV)
    xh = x.to(DEV, dtype)
    with torch.no_grad():
        y = module(R.ElementsToSummaryRepresentationInput(xh, idx.to(DEV), G))
        y32 = module(R.ElementsToSummaryRepresentationInput(xh.float(), idx.to(DEV), G))
    assert y.dtype == dtype
    assert float((y.float() - y32).abs().max()) <= 2e-2 * max(1.0, float(y32.abs().max()))


def exchange_case():
    torch.manual_seed(5)
    D, D2, G = 64, 32, 5
    pool = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, D2, 4, R.SimpleVarSizedElementReduce("max"))
    layer = R.GruGlobalStateUpdate(pool, D, D2)
    g = torch.Generator().manual_seed(6)
    idx = torch.repeat_interleave(torch.arange(G), torch.tensor([300, 1, 150, 40, 9]))
    x = torch.randn(idx.shape[0], D, generator=g)
    gout = torch.randn(idx.shape[0], D, generator=g)
    return layer, x, idx, gout


def test_gru_global_state_update_training_step_matches_float64_autograd():
    layer, x, idx, gout = exchange_case()
    cpu = {dt: copy.deepcopy(layer).to(dt) for dt in (torch.float32, torch.float64)}
    gpu = layer.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    before = ops.launch_counts(aggregation=True)
    y = gpu(xd, None, idx.to(DEV), None, None, None)
    y.backward(gout.to(DEV))
    ran = ops.launches_since(before)
    assert ran.get("attention_pool") == 1 and ran.get("attention_pool_backward") == 1, ran
    res = {}
    for dt, m in cpu.items():
        xr = x.detach().to(dt).clone().requires_grad_(True)
        yr = m(xr, None, idx, None, None, None)
        yr.backward(gout.to(dt))
        res[dt] = {"y": yr, "x": xr.grad}
        res[dt].update({k: p.grad for k, p in m.named_parameters()})
    got = {"y": y, "x": xd.grad}
    got.update({k: p.grad for k, p in gpu.named_parameters()})
    assert set(got) == set(res[torch.float64])
    for k, v in got.items():
        exact = res[torch.float64][k]
        assert attributed_ok(v, res[torch.float32][k], exact, TOL, max(1.0, float(exact.detach().abs().max()))), k


def test_forward_sharded_refuses_an_attention_pool():
    layer, x, idx, _ = exchange_case()
    layer = layer.to(DEV)
    shard = types.SimpleNamespace(node_to_graph_idx=idx.to(DEV), num_graphs=5, group=None, world=1)
    with pytest.raises(_lib.PtgnnAmdError, match="cannot combine partial pools"):
        layer.forward_sharded(x.to(DEV), shard)
