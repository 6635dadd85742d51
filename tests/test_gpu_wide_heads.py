"""The matrix-core attention pool and copy scores past 8 heads (csrc/wide_heads.hip) on the MI355X, behind
`ptgnn_amd.set_wide_heads`: the kernels, the multi-head reducer and the decoder against float64 restatements (the bars
and the attribution rule of tests/test_gpu_attention_pool.py and tests/test_gpu_decoder.py), launches and determinism."""
import math
from unittest import mock

import pytest
import torch

import ptgnn_amd
from agg_paths import TOL, attributed_ok
from decoder_cases import CASES, build, make_inputs, ref_loss, weights_of
from ptgnn_amd import ops, reduceops as R, scatter, sequence
from segment_batches import ref_attention_pool, ref_multihead, segment_lse

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
INF = float("inf")
SIZES = [300, 1, 0, 57, 129, 4]      # three chunks, a 1-row tile, an empty sample, a chunk boundary at 128 | 129
FAMILIES = ["wide_heads_pool", "wide_heads_pool_backward", "wide_heads_scores", "wide_heads_scores_backward"]


def attributed(got, want32, exact):
    return attributed_ok(got, want32, exact, TOL, max(1.0, float(exact.detach().abs().max())))


def segments(D, H, sizes, scale=1.0, shuffled=True):
    """idx over len(sizes) + 1 samples (the last one empty), rows x, vectors u, cotangents of [G, H, D], [n, H], [G, H]."""
    g = torch.Generator().manual_seed(9000 + 13 * D + H + sum(sizes))
    G = len(sizes) + 1
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffled:
        idx = idx[torch.randperm(idx.shape[0], generator=g)]
    x = torch.randn(idx.shape[0], D, generator=g) * scale
    u = torch.randn(G, H, D, generator=g) / (1.0 if scale != 1.0 else math.sqrt(D))
    cot = [torch.randn(G, H, D, generator=g), torch.randn(idx.shape[0], H, generator=g), torch.randn(G, H, generator=g)]
    return [t.to(DEV) for t in [idx, x, u] + cot] + [G]


# heads x D: odd / even K padding (D = 2 is one MFMA K step and fewer columns than waves), both head-block counts, U in
# LDS and (64 heads at D = 256, backward) read from global memory
@pytest.mark.parametrize("D,H,scale", [(2, 9, 1.0), (6, 33, 1.0), (7, 16, 1.0), (64, 9, 1.0), (64, 33, 8.0),
                                       (256, 64, 1.0), (512, 32, 1.0)])
def test_pool_kernel_against_float64(D, H, scale):
    idx, x, u, gp, _, _, G = segments(D, H, SIZES, scale)
    plan = ops.plan_for([(idx, idx)], G)
    before = ops.launch_counts(wide_heads=True)
    pooled, stats = ops.wide_heads_pool(x, u, plan)
    gx, gu = ops.wide_heads_pool_backward(x, u, plan, pooled, stats, gp)
    assert ops.launches_since(before) == {"wide_heads_pool": 1, "wide_heads_pool_backward": 1}
    empty = torch.tensor([s == 0 for s in SIZES] + [True], device=DEV)
    assert float(pooled[empty].abs().max()) == 0.0 and float(gu[empty].abs().max()) == 0.0
    res = {}
    for dt in (torch.float32, torch.float64):
        xr, ur = x.detach().to(dt).clone().requires_grad_(True), u.detach().to(dt).clone().requires_grad_(True)
        p, _, lse = ref_attention_pool(xr, idx, G, ur)
        p.backward(gp.to(dt))
        res[dt] = {"pooled": p.detach(), "lse": lse.detach()[~empty], "grad_x": xr.grad, "grad_u": ur.grad}
    if scale != 1.0:
        s = (u.double()[idx] * x.double().unsqueeze(1)).sum(-1)
        assert max(float(s[idx == b].max() - s[idx == b].min()) for b in (0, 3, 4)) > 100.0     # needs the running max
    got = {"pooled": pooled, "lse": stats[:, H:][~empty], "grad_x": gx, "grad_u": gu}
    for k, v in got.items():
        assert attributed(v, res[torch.float32][k], res[torch.float64][k]), k


@pytest.mark.parametrize("D", [6, 64])
@pytest.mark.parametrize("L", [9, 33, 64])
def test_scores_against_float64(D, L):
    idx, y, v, _, gs, gl, G = segments(D, L, SIZES)
    plan = ops.plan_for([(idx, idx)], G)
    yd, vd = y.clone().requires_grad_(True), v.clone().requires_grad_(True)
    empty = torch.tensor([s == 0 for s in SIZES] + [True], device=DEV)
    before = ops.launch_counts(aggregation=True, wide_heads=True)
    with ptgnn_amd.wide_heads():
        scores, lse = scatter.segment_scores(yd, vd, plan)
        ((scores * gs).sum() + (lse[~empty] * gl[~empty]).sum()).backward()
    assert ops.launches_since(before) == {"wide_heads_scores": 1, "wide_heads_scores_backward": 1}
    assert torch.equal(lse == -INF, empty.unsqueeze(1).expand(G, L))        # -inf exactly on the empty samples
    assert float(vd.grad[empty].abs().max()) == 0.0 and bool(torch.isfinite(yd.grad).all())
    res = {}
    for dt in (torch.float32, torch.float64):
        yr, vr = y.detach().to(dt).clone().requires_grad_(True), v.detach().to(dt).clone().requires_grad_(True)
        s = (vr[idx] * yr.unsqueeze(1)).sum(-1)
        l = segment_lse(s, idx, G)
        ((s * gs.to(dt)).sum() + (l[~empty] * gl.to(dt)[~empty]).sum()).backward()
        res[dt] = {"scores": s.detach(), "lse": l.detach()[~empty], "grad_y": yr.grad, "grad_v": vr.grad}
    got = {"scores": scores, "lse": lse[~empty], "grad_y": yd.grad, "grad_v": vd.grad}
    for k, val in got.items():
        assert attributed(val, res[torch.float32][k], res[torch.float64][k]), k


# through the public class hidden = D (a `max` query), so heads divide D: 9 and 33 heads at D = 18 and 66 (D = 2 (mod 4),
# no K padding; a 1- and a 2-wide head); D = 2, 6, 7 with 9 / 33 / 16 heads are test_pool_kernel_against_float64's
@pytest.mark.parametrize("D,H,value,scale", [(18, 9, False, 1.0), (66, 33, True, 1.0), (64, 16, False, 1.0),
                                             (64, 32, True, 1.0), (64, 64, False, 8.0), (256, 16, True, 1.0),
                                             (256, 64, False, 1.0)])
def test_multihead_reducer_against_float64(D, H, value, scale):
    g = torch.Generator().manual_seed(1000 + D * 17 + H)
    G = len(SIZES) + 1
    idx = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    idx = idx[torch.randperm(idx.shape[0], generator=g)].to(DEV)
    x, gout = (torch.randn(idx.shape[0], D, generator=g) * scale).to(DEV), torch.randn(G, 32, generator=g).to(DEV)
    torch.manual_seed(0)
    module = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, 32, H, R.SimpleVarSizedElementReduce("max"),
                                                           use_value_layer=value).to(DEV)
    xd = x.clone().requires_grad_(True)
    before = ops.launch_counts(aggregation=True, wide_heads=True)
    with ptgnn_amd.wide_heads(), mock.patch.object(torch.nn.functional, "linear", side_effect=AssertionError("F.linear")):
        y = module(R.ElementsToSummaryRepresentationInput(xd, idx, G))
        y.backward(gout)
    ran = ops.launches_since(before)       # fails without the feature: 9 .. 64 heads composed, whatever the switch said
    assert ran.get("wide_heads_pool") == 1 and ran.get("wide_heads_pool_backward") == 1 and "attention_pool" not in ran
    assert float(y[[2, G - 1]].abs().max()) == 0.0                                   # empty samples: exact zeros
    got = {"y": y, "x": xd.grad}
    got.update({k.split("__")[-1]: p.grad for k, p in module.named_parameters()})
    sd = {k.split("__")[-1]: v for k, v in module.state_dict().items()}
    res = {}
    for dt in (torch.float32, torch.float64):
        xr = x.detach().to(dt).clone().requires_grad_(True)
        w = [sd[k].detach().to(dt).requires_grad_(True) if k in sd else None
             for k in ("key_layer.weight", "value_layer.weight", "output_layer.weight")]
        yr, scores = ref_multihead(xr, idx, G, *w, H)
        yr.backward(gout.to(dt))
        res[dt] = {"y": yr, "x": xr.grad, "key_layer.weight": w[0].grad, "output_layer.weight": w[2].grad}
        if value:
            res[dt]["value_layer.weight"] = w[1].grad
    if scale != 1.0:
        assert max(float(scores[idx == b].max() - scores[idx == b].min()) for b in (0, 3, 4)) > 100.0
    assert set(got) == set(res[torch.float64])
    for k, v in got.items():
        assert attributed(v, res[torch.float32][k], res[torch.float64][k]), k


def decoder_run(spec, rate, method, on, seed=None):
    torch.manual_seed(31)
    module = build(spec, sequence, rate).to(DEV)
    inputs = {k: v.to(DEV) for k, v in make_inputs(spec, torch.Generator().manual_seed(32)).items()}
    inputs["input_memories"].requires_grad_(True)
    inputs["initial_states"].requires_grad_(True)
    if seed is not None:
        torch.manual_seed(seed)
    before = ops.launch_counts(aggregation=True, wide_heads=True)
    with ptgnn_amd.wide_heads(on):
        loss = getattr(module, method)(**inputs)
        loss.backward()
    grads = {"input_memories": inputs["input_memories"].grad, "initial_states": inputs["initial_states"].grad}
    grads.update({k: p.grad for k, p in module.named_parameters()})
    return module, inputs, loss.detach(), grads, ops.launches_since(before)


@pytest.mark.parametrize("method", ["forward", "fused_loss"])
@pytest.mark.parametrize("T", [10, 34])
def test_decoder_against_float64(T, method):
    module, inputs, loss, grads, ran = decoder_run(dict(CASES[0][1], T=T), 0.0, method, True)
    assert all(ran.get(f, 0) >= 1 for f in FAMILIES) and not {"segment_scores", "attention_pool"} & set(ran), ran
    res = {}
    for dt in (torch.float32, torch.float64):
        w = weights_of(module, dt)
        cast = {k: (v.detach().to(dt).requires_grad_(True) if v.is_floating_point() else v) for k, v in inputs.items()}
        want = ref_loss(w, **cast)
        want.backward()
        g = {"input_memories": cast["input_memories"].grad, "initial_states": cast["initial_states"].grad}
        g.update({k: w[k.split("__", 1)[1]].grad for k, _ in module.named_parameters()})
        res[dt] = (want.detach(), g)
    assert attributed(loss, res[torch.float32][0], res[torch.float64][0])
    for k, g in grads.items():
        assert attributed(g, res[torch.float32][1][k], res[torch.float64][1][k]), k


@pytest.mark.parametrize("method", ["forward", "fused_loss"])
@pytest.mark.parametrize("T", [10, 34])
def test_decoder_with_dropout_takes_the_projected_rows_and_repeats_under_one_seed(T, method):
    """Active dropout: rows = dropout(W_c x) [I, H], vectors = the GRU states; no float64 restatement draws the same
    masks, so the route is pinned by its launches, its row width, equal bits under one seed and other bits under another."""
    spec = dict(CASES[0][1], T=T)
    assert spec["H"] != spec["Dm"]
    with mock.patch.object(ops, "wide_heads_scores", wraps=ops.wide_heads_scores) as scores:
        runs = [decoder_run(spec, 0.2, method, True, seed=5) for _ in range(2)]
    assert [int(c.args[0].shape[1]) for c in scores.call_args_list] == [spec["H"]] * 2
    assert all(runs[0][4].get(f, 0) >= 1 for f in FAMILIES), runs[0][4]
    assert torch.equal(runs[0][2], runs[1][2]) and bool(torch.isfinite(runs[0][2]))
    for a, b in zip(runs[0][3].values(), runs[1][3].values()):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(runs[0][2], decoder_run(spec, 0.2, method, True, seed=6)[2])


def test_switch_off_launches_none_of_the_families_and_keeps_its_bits():
    runs = [decoder_run(dict(CASES[0][1], T=10), 0.0, "forward", False) for _ in range(2)]
    assert not set(FAMILIES) & set(runs[0][4]), runs[0][4]
    assert torch.equal(runs[0][2], runs[1][2])


def test_same_bits_twice_and_at_another_offset_in_a_larger_batch():
    D, H, sizes = 64, 33, [200, 57, 300, 40]
    idx, x, u, gp, _, _, G = segments(D, H, sizes, shuffled=False)
    plan = ops.plan_from_sorted_index(idx, G)
    runs = []
    for _ in range(2):
        pooled, stats = ops.wide_heads_pool(x, u, plan)
        runs.append((pooled, stats) + ops.wide_heads_pool_backward(x, u, plan, pooled, stats, gp))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    rows = torch.nonzero(idx == 2).flatten()
    x1, u1, gp1 = x[rows].contiguous(), u[2:3].contiguous(), gp[2:3].contiguous()
    plan1 = ops.plan_from_sorted_index(torch.zeros_like(rows), 1)
    pooled1, stats1 = ops.wide_heads_pool(x1, u1, plan1)
    gx1, gu1 = ops.wide_heads_pool_backward(x1, u1, plan1, pooled1, stats1, gp1)
    pooled, stats, gx, gu = runs[0]
    assert torch.equal(pooled[2], pooled1[0]) and torch.equal(stats[2], stats1[0])
    assert torch.equal(gx[rows], gx1) and torch.equal(gu[2], gu1[0])
