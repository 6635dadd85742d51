"""The panel-form 16-bit Linear on the GPU (csrc/panel_linear16.hip, the masked form of csrc/wgrad16.hip; reached through
`ptgnn_amd.set_attention_training(True, linears=True)`): the forward against the existing 16-bit Linear (same chain, same
bits), float64 on the rounded operands and an exact integer case; the epilogue's dropout and addend against torch on the
p = 0 launch; the masked input and weight gradients against the unfused pair (act_dropout_backward + the plain 16-bit
GEMMs), bit for bit; the autograd node; and the attention layer's training step against the step spelled from the nodes.

Shapes: the smallest at which the kernel can go wrong -- rows around the 64-row wave split and the 128-row tile, k of
half a panel to three panels, n_out of one sub-tile to two column tiles; 545 rows put the weight gradient one panel past
its 512-row chunk, so the two-stage reduction runs."""
import pytest
import torch

import half_cases as C
from helpers import dropout_keep_scale
from selfatt_cases import PREFIX

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
DEV = torch.device("cuda")
SEED = (5 << 40) + 987
# (rows, k, n_out, act, strided views)
CASES = [(1, 32, 32, None, False), (65, 64, 96, "relu", False), (128, 96, 128, "tanh", False),
         (129, 192, 160, "relu", False), (300, 64, 256, None, True), (300, 192, 32, "tanh", False),
         (65, 32, 256, "relu", True), (545, 96, 128, "relu", False)]
SHAPES = pytest.mark.parametrize("case", CASES, ids=lambda c: f"r{c[0]}k{c[1]}n{c[2]}-{c[3]}" + ("-strided" if c[4] else ""))


def _on_gpu(t, strided):
    """`t` on the GPU; `strided`: as a column slice of a buffer 8 floats wider (ld greater than the width)."""
    if not strided:
        return t.to(DEV)
    buf = torch.zeros(t.shape[0], t.shape[1] + 8, device=DEV)
    buf[:, 4:4 + t.shape[1]] = t.to(DEV)
    return buf[:, 4:4 + t.shape[1]]


def _operands(case):
    rows, k, n_out, _, strided = case
    g = torch.Generator().manual_seed(7700 + rows + k + n_out)
    x, grad, add = (torch.randn(rows, w, generator=g) for w in (k, n_out, n_out))
    return (_on_gpu(x, strided), C.xavier(n_out, k, g).to(DEV), (torch.randn(n_out, generator=g) * 0.1).to(DEV),
            _on_gpu(grad, strided), _on_gpu(add, strided))


def _unfused_backward(x, w, grad, y, act, p, dt):
    """(d_x, d_w, d_b) from the pass the panel launches fold away: act_dropout_backward, then the plain 16-bit GEMMs."""
    from ptgnn_amd import ops
    rows, n_out = grad.shape
    keep = (dropout_keep_scale(SEED, rows, n_out, p) > 0).to(DEV) if p > 0 else None
    g1 = ops.act_dropout_backward(grad.contiguous(), y, keep, 1.0 / (1.0 - p), act)
    return (g1, ops.linear(g1, w.t().contiguous(), inputs=dt)) + ops.half_linear_weight_grad(x, g1, dt, want_bias=True)


@DTYPES
@SHAPES
def test_forward_has_the_bits_of_the_16_bit_linear_and_is_within_the_bar_of_float64(case, dt):
    from ptgnn_amd import ops
    x, w, b, _, _ = _operands(case)
    for act in (None, "relu", "tanh"):
        before = ops.launch_counts(panel16=True)
        y = ops.panel_linear16(x, w, b, act, dt)
        assert ops.launches_since(before) == {"panel_linear16": 1}
        want = C.linear64(x, w, b, act, dt)
        print(case, act, "err", C.err(y, want), "bar", C.bar(want))
        assert torch.equal(y, ops.linear(x, w, b, act=act, inputs=dt)) and C.err(y, want) <= C.bar(want)


@DTYPES
@SHAPES
def test_integer_case_is_exact_forward_and_in_the_masked_input_gradient(case, dt):
    from ptgnn_amd import ops
    rows, k, n_out, _, _ = case
    x, w, b = (t.to(DEV) for t in C.integer_case(rows, k, n_out, 7800 + rows))
    y = ops.panel_linear16(x, w, b, "relu", dt)
    assert torch.equal(y.cpu().double(), torch.relu(x.cpu().double() @ w.cpu().double().t() + b.cpu().double()))
    grad = torch.randint(-4, 5, (rows, n_out), generator=torch.Generator().manual_seed(7801)).float().to(DEV)
    d_x = ops.panel_linear16_grad_input(grad, y, w.t().contiguous(), "relu", dt, p=0.5, seed=SEED)
    g1 = grad.cpu().double() * dropout_keep_scale(SEED, rows, n_out, 0.5).double() * (y.cpu() > 0)
    assert torch.equal(d_x.cpu().double(), g1 @ w.cpu().double())


@DTYPES
@SHAPES
def test_dropout_and_addend_of_the_epilogue_equal_torch_on_the_launch_without_them(case, dt):
    from ptgnn_amd import ops
    rows, _, n_out, act, _ = case
    x, w, b, _, add = _operands(case)
    y0 = ops.panel_linear16(x, w, b, act, dt)
    y, y_act = ops.panel_linear16(x, w, b, act, dt, p=0.25, seed=SEED, addend=add, want_act=True)
    assert torch.equal(y, y0 * dropout_keep_scale(SEED, rows, n_out, 0.25).to(DEV) + add) and torch.equal(y_act, y0)
    assert torch.equal(y, ops.panel_linear16(x, w, b, act, dt, p=0.25, seed=SEED, addend=add))
    assert not torch.equal(y, ops.panel_linear16(x, w, b, act, dt, p=0.25, seed=SEED + 1, addend=add))


@DTYPES
@SHAPES
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_masked_gradients_and_the_node_have_the_bits_of_the_unfused_backward(case, dt, p):
    from ptgnn_amd import dense, ops
    rows, k, n_out, act, _ = case
    x, w, b, grad, add = _operands(case)
    y = ops.panel_linear16(x, w, b, act, dt)
    g1, d_x, d_w, d_b = _unfused_backward(x, w, grad, y, act, p, dt)
    got_x = ops.panel_linear16_grad_input(grad, y, w.t().contiguous(), act, dt, p=p, seed=SEED)
    want = C.rnd64(g1, dt) @ C.rnd64(w, dt)
    print(case, p, "d_x err", C.err(got_x, want), "bar", C.bar(want))
    assert torch.equal(got_x, d_x) and C.err(got_x, want) <= C.bar(want)
    got_w, got_b = ops.half_linear_weight_grad_masked(x, grad, y, act, dt, p=p, seed=SEED, want_bias=True)
    assert torch.equal(got_w, d_w) and torch.equal(got_b, d_b)
    assert (ops.half_wgrad_chunk_rows(rows, n_out, k) < rows) == (rows == 545)      # the two-stage reduction ran
    leaves = [t.clone().requires_grad_() for t in (x, w, b, add)]
    out = dense.linear_act_dropout(*leaves[:3], act, p, True, inputs=dt, seed=SEED, addend=leaves[3])
    node = torch.autograd.grad(out, leaves, grad)
    assert all(torch.equal(u, v) for u, v in zip(node, (d_x, d_w, d_b, grad)))


COUNTS, MAX_NODES, D, HEADS, DK, DV, INTER = [5, 40, 70], 70, 64, 2, 32, 32, 128


def _train_step(layer, forward):
    torch.manual_seed(9702)                 # the dropout seeds are drawn from torch's CPU generator
    layer.zero_grad()
    y = forward()
    y.square().sum().backward()
    return [y.detach().clone()] + [q.grad.clone() for q in layer.parameters()]


@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_training_step_under_the_keyword_equals_the_step_spelled_from_the_nodes(dt, p):
    import ptgnn_amd
    from ptgnn_amd import dense, layers as L, ops, scatter
    torch.manual_seed(9700)
    layer = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, dropout_rate=p,
                                                   max_num_nodes=MAX_NODES).to(DEV).train()
    x = torch.randn(sum(COUNTS), D, generator=torch.Generator().manual_seed(9701)).to(DEV)
    idx = torch.repeat_interleave(torch.arange(len(COUNTS)), torch.tensor(COUNTS)).to(DEV)
    w_h, w_s, w_i, w_o, ln1, ln2 = (getattr(layer, PREFIX + n) for n in (
        "selfatt_head_transforms", "summarization_layer", "intermediate_layer", "output_layer", "layer_norm1",
        "layer_norm2"))
    # precondition on the inputs: the fp32 Linear is MARGIN bars from float64 on the rounded operands, the panel launch
    # within one -- so a step that quietly ran the fp32 node cannot equal the 16-bit one below
    want = C.linear64(x, w_i.weight, w_i.bias, "relu", dt)
    assert C.err(ops.linear(x, w_i.weight.detach(), w_i.bias.detach(), act="relu"), want) >= C.MARGIN * C.bar(want)
    assert C.err(ops.panel_linear16(x, w_i.weight.detach(), w_i.bias.detach(), "relu", dt), want) <= C.bar(want)

    def composed():
        seed = L._dropout_seed() if p > 0 else 0
        windows = ops.attention_windows(ops.plan_for([(idx, idx)], len(COUNTS)), MAX_NODES)
        kqv = dense.linear(x, w_h.weight, inputs=dt)
        values = scatter.block_attention(kqv, windows, MAX_NODES, HEADS, DK, DV, p, seed, inputs=dt)
        a = dense.row_epilogue(dense.linear_act_dropout(values, w_s.weight, None, None, p, p > 0, inputs=dt, seed=seed + 1,
                                                        addend=x), False, ln1)
        hidden = dense.linear_act_dropout(a, w_i.weight, w_i.bias, "relu", 0.0, False, inputs=dt, seed=seed + 2)
        return dense.row_epilogue(dense.linear_act_dropout(hidden, w_o.weight, w_o.bias, None, p, p > 0, inputs=dt,
                                                           seed=seed + 3, addend=a), False, ln2)

    run = lambda: layer(x, [], idx, {}, {}, [])      # noqa: E731
    panel_launches = lambda before: {n: c for n, c in ops.launches_since(before).items()     # noqa: E731
                                     if n in ("panel_linear16", "panel_linear16_grad_input", "half_wgrad_masked")}
    with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training():
        before = ops.launch_counts(panel16=True)
        plain = _train_step(layer, run)
        assert not panel_launches(before)                             # the plain switch: no panel launch
    with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training(linears=True):
        before = ops.launch_counts(panel16=True)
        got = _train_step(layer, run)
        since = panel_launches(before)
        want = _train_step(layer, composed)
    assert since == {"panel_linear16": 3, "panel_linear16_grad_input": 3, "half_wgrad_masked": 3 if p > 0 else 1}, since
    assert all(bool(torch.isfinite(t).all()) for t in got) and all(torch.equal(u, v) for u, v in zip(got, want))
    assert all(not torch.equal(u, v) for u, v in zip(got[1:], plain[1:]))    # every parameter's gradient moved
