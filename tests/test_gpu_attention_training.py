"""The 16-bit attention training step on the GPU (`ptgnn_amd.set_attention_training`; csrc/block_attention16.hip with
dropout, csrc/block_attention16_backward.hip): the op against the float64 restatement on the rounded operands inside the
DERIVED bounds of tests/attention_training_cases.py at every element, with the fp32 route at least twice outside them;
bits, the dropped set and placement; and the layer's training step under the switch, bit for bit against the same step
spelled from the autograd nodes, with everyone without the switch keeping their bits."""
import pytest
import torch

import attention_training_cases as T
import half_cases as C
import mlp_half_cases as MC
from selfatt_cases import PREFIX

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
DEV = torch.device("cuda")


def _launches(fn):
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, half=True, half_training=True, attention16=True, attention16_training=True)
    out = fn()
    return out, ops.launches_since(before)


def _windows(counts, max_num_nodes):
    from ptgnn_amd import ops
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(DEV)
    return ops.attention_windows(ops.plan_for([(idx, idx)], len(counts)), max_num_nodes)


def _view(t, pad=0, left=0):
    """`t` on the GPU as a column slice of a wider buffer: `pad` = 0 rounds the row stride up to 16 bytes (the condition
    of the 16-bit launches), else adds `pad` floats to it; `left` = first column of the slice."""
    buf = torch.zeros(t.shape[0], (t.shape[1] + 3) // 4 * 4 if pad == 0 else t.shape[1] + pad, device=DEV)
    buf[:, left:left + t.shape[1]] = t.to(DEV)
    return buf[:, left:left + t.shape[1]]


def _step(kqv, gout, counts, max_nodes, heads, dk, dv, p=0.0, seed=0, inputs=None):
    """(out, lse, grad_kqv) of the op pair the autograd node runs."""
    from ptgnn_amd import ops
    w = _windows(counts, max_nodes)
    out, lse = ops.block_attention(kqv, w, max_nodes, heads, dk, dv, p, seed, inputs=inputs, masked16=True)
    return out, lse, ops.block_attention_backward(kqv, out, lse, gout.to(DEV), w, max_nodes, heads, dk, dv, p, seed,
                                                  inputs=inputs)


@DTYPES
@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_op_is_inside_the_derived_bounds_of_the_rounded_reference_and_the_fp32_route_is_not(c, dt):
    _, heads, dk, dv, p, _ = c
    ref = T.case(c, dt)
    want, hw = ref["rounded"], 2 * dk + dv
    args = (_view(ref["kqv"]), ref["gout"], ref["counts"], ref["max"], heads, dk, dv, p, T.SEED)
    (out, _, grad), since = _launches(lambda: _step(*args, inputs=dt))
    assert since == {"attention_train16" if p > 0 else "block_attention16": 1, "attention_train16_backward": 1}, since
    out, grad = out.cpu(), grad.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    figures = {"out": T.worst(out, want["out"], want["out_bound"])}
    cols = torch.arange(heads * hw) % hw
    for name, lo, hi in (("d_key", 0, dk), ("d_query", dk, 2 * dk), ("d_value", 2 * dk, hw)):
        sel = (cols >= lo) & (cols < hi)
        figures[name] = T.worst(grad[:, sel], want["grad"][:, sel], want["grad_bound"][:, sel])
    far = T.worst(_step(*args)[2].cpu(), want["grad"], want["grad_bound"])
    print(f"max |got - rounded| / bound: {figures}; the fp32 route: {far:.2f}")
    assert all(v <= 1.0 for v in figures.values()), figures
    assert far >= 2.0, far


@DTYPES
def test_bits_of_the_forward_the_dropped_set_strided_rows_and_two_runs(dt):
    from ptgnn_amd import ops
    heads, dk, dv = 2, 16, 16
    counts, max_nodes = T.BATCHES["max33"]
    kqv = T.make_kqv(counts, heads, dk, dv, 9300).to(DEV)
    gout = torch.randn(kqv.shape[0], heads * dv, generator=torch.Generator().manual_seed(9301))
    shape = (counts, max_nodes, heads, dk, dv)
    inference = ops.block_attention(kqv, _windows(counts, max_nodes), max_nodes, heads, dk, dv, inputs=dt)
    assert all(torch.equal(x, y) for x, y in zip(_step(kqv, gout, *shape, inputs=dt), inference))   # p = 0: those bits
    flat = kqv.clone()                     # small keys: every probability is about 1 / n, so every flipped keep shows
    flat.view(-1, heads, 2 * dk + dv)[..., :dk] *= 0.01
    moved = [torch.ne(*(_step(flat, gout, *shape, 0.25, s, inputs)[0] for s in (11, 12))) for inputs in (None, dt)]
    assert torch.equal(*moved) and bool(moved[0].any())        # positions of `out` that move with the seed: both routes
    got = _step(kqv, gout, *shape, 0.25, 11, dt)
    assert all(torch.equal(x, y) for x, y in zip(got, _step(kqv, gout, *shape, 0.25, 11, dt)))      # two runs
    assert all(torch.equal(x, y) for x, y in zip(got, _step(_view(kqv, 8, 4), gout, *shape, 0.25, 11, dt)))  # other stride
    strided, since = _launches(lambda: _step(_view(kqv, 1), gout, *shape, 0.25, 11, dt))    # rows 97 floats apart: fp32
    assert since == {"block_attention": 1, "block_attention_backward": 1}, since
    assert all(torch.equal(x, y) for x, y in zip(strided, _step(kqv, gout, *shape, 0.25, 11)))


@DTYPES
@pytest.mark.parametrize("dk,dv", [(32, 32), (17, 6)], ids=["k32v32", "k17v6"])
def test_a_window_gives_the_same_gradient_bits_first_in_the_middle_and_last_in_a_batch(dt, dk, dv):
    heads, sizes, max_nodes = 3, (70, 5, 31), 33          # 70 -> windows of 33, 33 and 4 rows
    kqv = T.make_kqv([sum(sizes)], heads, dk, dv, 9400 + dk)
    gout = torch.randn(kqv.shape[0], heads * dv, generator=torch.Generator().manual_seed(9401))
    k, g = kqv.split(sizes), gout.split(sizes)
    got = []
    for order in ((0, 1, 2), (1, 0, 2), (1, 2, 0)):
        first = sum(sizes[i] for i in order[:order.index(0)])
        res = _step(_view(torch.cat([k[i] for i in order])), torch.cat([g[i] for i in order]), [sizes[i] for i in order],
                    max_nodes, heads, dk, dv, inputs=dt)
        got.append([t[first:first + sizes[0]].clone() for t in res])
    assert all(torch.equal(x, y) for other in got[1:] for x, y in zip(other, got[0]))


COUNTS, MAX_NODES, D, HEADS, DK, DV, INTER = [40, 33, 5], 33, 64, 2, 16, 16, 128


def _layer(p):
    from ptgnn_amd import layers as L
    torch.manual_seed(9500)
    layer = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, dropout_rate=p, max_num_nodes=MAX_NODES)
    x = torch.randn(sum(COUNTS), D, generator=torch.Generator().manual_seed(9501)).to(DEV)
    return layer.to(DEV), x, torch.repeat_interleave(torch.arange(len(COUNTS)), torch.tensor(COUNTS)).to(DEV)


def _train_step(layer, forward):
    torch.manual_seed(9502)                 # the dropout seeds are drawn from torch's CPU generator
    layer.zero_grad()
    y = forward()
    y.square().sum().backward()
    return [y.detach().clone()] + [p.grad.clone() for p in layer.parameters()]


def _composed(layer, x, p, dt):
    """The training forward spelled from the autograd nodes: the 16-bit Linear and attention nodes, the fp32 others."""
    from ptgnn_amd import dense, layers as L, scatter
    w_h, w_s, w_i, w_o, ln1, ln2 = (getattr(layer, PREFIX + n) for n in (
        "selfatt_head_transforms", "summarization_layer", "intermediate_layer", "output_layer", "layer_norm1",
        "layer_norm2"))
    seed = L._dropout_seed() if p > 0 else 0
    kqv = dense.linear(x, w_h.weight, inputs=dt)
    values = scatter.block_attention(kqv, _windows(COUNTS, MAX_NODES), MAX_NODES, HEADS, DK, DV, p, seed, inputs=dt)
    a = dense.row_epilogue(dense.linear_act_dropout(values, w_s.weight, None, None, p, p > 0) + x, False, ln1)
    hidden = dense.linear_act_dropout(a, w_i.weight, w_i.bias, "relu", 0.0, False)
    return dense.row_epilogue(dense.linear_act_dropout(hidden, w_o.weight, w_o.bias, None, p, p > 0) + a, False, ln2)


@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_training_step_under_the_switch_equals_the_step_spelled_from_the_nodes(dt, p):
    import ptgnn_amd
    layer, x, idx = _layer(p)
    run = lambda: layer.train()(x, [], idx, {}, {}, [])      # noqa: E731
    plain = _train_step(layer, run)
    with ptgnn_amd.matrix_inputs(dt, attention=True):                       # without the switch: today's fp32 bits
        off, since = _launches(lambda: _train_step(layer, run))
    assert all(torch.equal(u, v) for u, v in zip(off, plain)) and "attention_train16_backward" not in since, since
    with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training():
        got, since = _launches(lambda: _train_step(layer, run))
        want = _train_step(layer, lambda: _composed(layer, x, p, dt))
    assert since.get("attention_train16" if p > 0 else "block_attention16") == 1, since
    assert since.get("attention_train16_backward") == 1 and since.get("half_linear", 0) >= 1, since
    assert "block_attention" not in since and "block_attention_backward" not in since, since
    assert all(bool(torch.isfinite(g).all()) for g in got) and all(torch.equal(u, v) for u, v in zip(got, want))
    assert all(not torch.equal(u, v) for u, v in zip(got[1:], plain[1:]))    # every parameter's gradient moved


@DTYPES
def test_inference_and_the_other_layers_do_not_follow_the_switch(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    layer, x, idx = _layer(0.1)
    torch.manual_seed(9600)
    ggnn = L.GatedMessagePassingLayer(64, 64, 8, "sum").eval().cuda()
    gx = torch.randn(300, 64, generator=torch.Generator().manual_seed(9601)).cuda()
    adj = [(s.cuda(), d.cuda()) for s, d in C.random_adjacency(300, (25,) * 8, 9602)]
    key = ("table", 64, "sum", True)
    mlp, mx, madj = MC.layer_case(*key, MC.LAYER_SEEDS[key])
    others = ((ggnn, gx, adj), (mlp.cuda(), mx.cuda(), [(s.cuda(), d.cuda()) for s, d in madj]))
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt):
        plain = layer.eval()(x, [], idx, {}, {}, [])
        wants = [MC.run_layer(*o) for o in others]
        with ptgnn_amd.attention_training():
            got, since = _launches(lambda: layer(x, [], idx, {}, {}, []))
            assert torch.equal(got, plain) and since.get("block_attention") == 1 and "block_attention16" not in since, since
            for want, o in zip(wants, others):
                flagged, since = _launches(lambda: MC.run_layer(*o))
                assert torch.equal(flagged, want) and not [k for k in since if "attention" in k], since
