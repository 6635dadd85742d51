"""The 16-bit matrix-core inputs of the attention layer on the GPU (ptgnn_amd/precision.py `attention=True`,
csrc/block_attention16.hip): the op against the float64 restatement on the rounded operands inside the DERIVED bound of
tests/attention_inputs_cases.py (every element), with the precondition -- asserted from the two float64 references
alone -- that the exact-fp32 result lies far outside that bound, so a route that quietly ran the fp32 kernel fails;
placement independence; the dispatch of `ops.block_attention(inputs=)`; the layer under the flag, bit for bit against
the same sequence composed from the ops; and everyone without the flag keeping their bits."""
import pytest
import torch

import attention_inputs_cases as A
import half_cases as C
import mlp_half_cases as MC
from dense_paths import TOL
from selfatt_cases import PREFIX, TARGET

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
DEV = torch.device("cuda")


def _launches(fn):
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, half=True, half_training=True, attention16=True)
    out = fn()
    return out, ops.launches_since(before)


def _windows(counts, max_num_nodes):
    from ptgnn_amd import ops
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(DEV)
    return ops.attention_windows(ops.plan_for([(idx, idx)], len(counts)), max_num_nodes)


def _attend(kqv, counts, max_num_nodes, heads, dk, dv, **kw):
    from ptgnn_amd import ops
    return ops.block_attention(kqv.to(DEV), _windows(counts, max_num_nodes), max_num_nodes, heads, dk, dv, **kw)


def _aligned_rows(kqv):
    """`kqv` on the GPU as a view whose rows are 16 bytes apart or a multiple of that (the condition of the 16-bit
    launch): heads (2 dk + dv) = 3 or 9 floats at dk = dv = 1 is no such stride by itself."""
    n, width = kqv.shape
    buf = torch.zeros(n, (width + 3) // 4 * 4, device=DEV)
    buf[:, :width] = kqv.to(DEV)
    return buf[:, :width]


# ---------------------------------------------------------------------------------------------------------------------
# op numerics
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("batch", list(A.BATCHES))
@pytest.mark.parametrize("heads", A.HEADS)
@pytest.mark.parametrize("dk,dv", A.WIDTHS, ids=[f"k{k}v{v}" for k, v in A.WIDTHS])
def test_op_is_inside_the_derived_bound_of_the_rounded_reference_at_every_element(dt, batch, heads, dk, dv):
    c = A.case(batch, heads, dk, dv, dt)
    if dk >= 8:   # from the two float64 references alone: the fp32 kernel's result would fail below
        far, share = A.precondition(c)
        print(f"precondition: max |exact - rounded| / bound = {far:.2f}, outside = {share:.3f}")
        assert far >= 4.0 and share >= 0.10, (far, share)
    kqv = _aligned_rows(c["kqv"])
    (out, lse), since = _launches(lambda: _attend(kqv, c["counts"], c["max"], heads, dk, dv, inputs=dt))
    assert since == {"block_attention16": 1}, since
    out, lse = out.cpu().double(), lse.cpu().double()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    ratio = (out - c["rounded"]).abs() / c["bound"]
    lse_err = float((lse - c["lse"]).abs().max()) / max(1.0, float(c["lse"].abs().max()))
    print(f"max |got - rounded| / bound = {float(ratio.max()):.3f}, lse error / TOL = {lse_err / TOL:.3f}")
    assert float(ratio.max()) <= 1.0, f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside the bound"
    assert lse_err <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("dk,dv", [(32, 32), (17, 6)], ids=["k32v32", "k17v6"])
def test_a_window_gives_the_same_bits_first_in_the_middle_and_last_in_a_batch(dt, dk, dv):
    heads, own, others, max_nodes = 3, 70, (5, 31), 33          # 70 -> windows of 33, 33 and 4 rows
    kqv = A.make_kqv([own + sum(others)], heads, dk, dv, 7700 + dk)
    mine, a, b = kqv[:own], kqv[own:own + others[0]], kqv[own + others[0]:]
    got = []
    for order, first in (((mine, a, b), 0), ((a, mine, b), others[0]), ((a, b, mine), sum(others))):
        out, lse = _attend(torch.cat(order), [t.shape[0] for t in order], max_nodes, heads, dk, dv, inputs=dt)
        got.append((out[first:first + own].clone(), lse[first:first + own].clone()))
    for out, lse in got[1:]:
        assert torch.equal(out, got[0][0]) and torch.equal(lse, got[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_inputs_keyword_launches_the_16_bit_kernel_and_everything_else_the_fp32_one(dt):
    heads, dk, dv = 2, 16, 16
    counts, max_nodes = A.BATCHES["max33"]
    kqv = A.make_kqv(counts, heads, dk, dv, 7800).to(DEV)
    plain, since = _launches(lambda: _attend(kqv, counts, max_nodes, heads, dk, dv))
    assert since == {"block_attention": 1}, since
    half, since = _launches(lambda: _attend(kqv, counts, max_nodes, heads, dk, dv, inputs=dt))
    assert since == {"block_attention16": 1}, since
    assert not torch.equal(half[0], plain[0])
    for kw in ({"inputs": None}, {"inputs": torch.float32}):
        got, since = _launches(lambda: _attend(kqv, counts, max_nodes, heads, dk, dv, **kw))
        assert since == {"block_attention": 1} and torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), since
    dropped = _attend(kqv, counts, max_nodes, heads, dk, dv, p=0.25, seed=99)
    got, since = _launches(lambda: _attend(kqv, counts, max_nodes, heads, dk, dv, p=0.25, seed=99, inputs=dt))
    assert since == {"block_attention": 1} and torch.equal(got[0], dropped[0]) and torch.equal(got[1], dropped[1]), since
    wide = torch.zeros(kqv.shape[0], kqv.shape[1] + 1, device=DEV)       # a row stride of 97 floats: not 16-byte aligned
    wide[:, :kqv.shape[1]] = kqv
    view = wide[:, :kqv.shape[1]]
    assert view.stride(0) % 4 != 0
    got, since = _launches(lambda: _attend(view, counts, max_nodes, heads, dk, dv, inputs=dt))
    assert since == {"block_attention": 1} and torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), since


# ---------------------------------------------------------------------------------------------------------------------
# the layer under the flag
# ---------------------------------------------------------------------------------------------------------------------
COUNTS, MAX_NODES, D, HEADS, DK, DV, INTER = [40, 33, 5], 33, 64, 2, 16, 16, 128


def _layer(target=False, p=0.0, seed=8100):
    from ptgnn_amd import layers as L
    torch.manual_seed(seed)
    return L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, dropout_rate=p, max_num_nodes=MAX_NODES,
                                                  target_reference=TARGET if target else "all").to(DEV)


def _states(seed=8101):
    x = torch.randn(sum(COUNTS), D, generator=torch.Generator().manual_seed(seed)).to(DEV)
    idx = torch.repeat_interleave(torch.arange(len(COUNTS)), torch.tensor(COUNTS)).to(DEV)
    return x, idx


def _composed(layer, x, residual, dt):
    """The inference forward spelled from the ops with inputs=dt: what the layer must equal bit for bit."""
    from ptgnn_amd import ops
    w_h, w_s, w_i, w_o, ln1, ln2 = (getattr(layer, PREFIX + n) for n in (
        "selfatt_head_transforms", "summarization_layer", "intermediate_layer", "output_layer", "layer_norm1",
        "layer_norm2"))
    kqv = ops.linear(x, w_h.weight, inputs=dt)
    values, _ = ops.block_attention(kqv, _windows(COUNTS, MAX_NODES), MAX_NODES, HEADS, DK, DV, inputs=dt)
    a = ops.row_epilogue(ops.linear_add(values, w_s.weight, residual, inputs=dt), ops.EPI_LAYERNORM, ln1.weight,
                         ln1.bias, ln1.eps)
    hidden = ops.linear(a, w_i.weight, w_i.bias, act="relu", inputs=dt)
    return ops.row_epilogue(ops.linear_add(hidden, w_o.weight, a, bias=w_o.bias, inputs=dt), ops.EPI_LAYERNORM,
                            ln2.weight, ln2.bias, ln2.eps)


def _sixteen_bit_log(since):
    assert since.get("block_attention16") == 1 and "block_attention" not in since, since
    assert since.get("half_linear") == 2 and since.get("half_linear_add") == 2, since


@DTYPES
def test_layer_under_the_flag_equals_the_sequence_composed_from_the_ops(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer().eval(), _states()
    with torch.no_grad():
        default = layer(x, [], idx, {}, {}, [])
        with ptgnn_amd.matrix_inputs(dt, attention=True):
            got, since = _launches(lambda: layer(x, [], idx, {}, {}, []))
        assert ptgnn_amd.attention_inputs(x) is torch.float32
        want = _composed(layer, x, x, dt)
    _sixteen_bit_log(since)
    assert torch.equal(got, want) and not torch.equal(got, default) and bool(torch.isfinite(got).all())


@DTYPES
def test_layer_under_the_flag_with_a_permuted_target_reference(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer(target=True).eval(), _states()
    ids = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(8102)).to(DEV)
    unused = torch.zeros(x.shape[0], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        with ptgnn_amd.matrix_inputs(dt, attention=True):
            got, since = _launches(lambda: layer(x, [], unused, {TARGET: ids}, {TARGET: idx}, []))
        want = x.index_copy(0, ids, _composed(layer, x[ids], x, dt))
    _sixteen_bit_log(since)
    assert torch.equal(got, want)


@DTYPES
def test_layer_under_the_flag_with_bf16_states_returns_bf16(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer().eval(), _states()
    xb = x.to(torch.bfloat16)
    with torch.no_grad():
        with ptgnn_amd.matrix_inputs(dt, attention=True):
            got, since = _launches(lambda: layer(xb, [], idx, {}, {}, []))
        want = _composed(layer, xb.float(), xb.float(), dt).to(torch.bfloat16)
    _sixteen_bit_log(since)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


@DTYPES
def test_layer_follows_autocast_with_the_flag(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer().eval(), _states()
    try:
        ptgnn_amd.set_matrix_inputs("autocast", attention=True)
        with torch.no_grad():
            outside = layer(x, [], idx, {}, {}, [])
            with torch.autocast("cuda", dtype=dt):
                got, since = _launches(lambda: layer(x, [], idx, {}, {}, []))
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    with torch.no_grad():
        assert torch.equal(outside, layer(x, [], idx, {}, {}, []))      # no autocast region: fp32 bits
        want = _composed(layer, x, x, dt)
    _sixteen_bit_log(since)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# everyone else keeps their bits
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_settings_without_the_flag_leave_the_layer_at_its_fp32_bits(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer().eval(), _states()
    with torch.no_grad():
        default = layer(x, [], idx, {}, {}, [])
        for args, kw in (((dt,), {}), ((dt,), dict(edge_gemm=True, training=True, mlp=True)),
                         ((torch.float32,), dict(attention=True))):
            with ptgnn_amd.matrix_inputs(*args, **kw):
                got, since = _launches(lambda: layer(x, [], idx, {}, {}, []))
            assert torch.equal(got, default), kw
            assert since.get("block_attention") == 1 and "block_attention16" not in since, since
            assert "half_linear" not in since and "half_linear_add" not in since, since


@DTYPES
def test_a_call_that_needs_gradients_stays_fp32_under_the_flag(dt):
    import ptgnn_amd
    layer, (x, idx) = _layer().train(), _states()          # dropout 0: train() only asks for gradients

    def step():
        layer.zero_grad()
        y = layer(x, [], idx, {}, {}, [])
        y.square().sum().backward()
        return y.detach().clone(), [p.grad.clone() for p in layer.parameters()]

    y0, g0 = step()
    with ptgnn_amd.matrix_inputs(dt, attention=True):
        (y1, g1), since = _launches(step)
    assert "block_attention16" not in since and "half_linear" not in since, since
    assert torch.equal(y1, y0) and all(torch.equal(u, v) for u, v in zip(g1, g0))


@DTYPES
def test_ggnn_and_mlp_layers_do_not_follow_the_attention_flag(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(8200)
    ggnn = L.GatedMessagePassingLayer(64, 64, 8, "sum").eval().cuda()
    x = torch.randn(300, 64, generator=torch.Generator().manual_seed(8201)).cuda()
    adj = [(s.cuda(), d.cuda()) for s, d in C.random_adjacency(300, (25,) * 8, 8202)]
    key = ("table", 64, "sum", True)
    mlp, mx, madj = MC.layer_case(*key, MC.LAYER_SEEDS[key])
    mlp, mx, madj = mlp.cuda(), mx.cuda(), [(s.cuda(), d.cuda()) for s, d in madj]
    with torch.no_grad():
        for layer, xs, adjs in ((ggnn, x, adj), (mlp, mx, madj)):
            with ptgnn_amd.matrix_inputs(dt):
                plain = MC.run_layer(layer, xs, adjs)
            with ptgnn_amd.matrix_inputs(dt, attention=True):
                flagged, since = _launches(lambda: MC.run_layer(layer, xs, adjs))
            assert torch.equal(flagged, plain) and "block_attention16" not in since, since
