"""The opt-in 16-bit matrix inputs of the GGNN edge-form training step on the MI355X: the masked forms of
csrc/edge_gemm16.hip through the C entry (strided output) and `ops.edge_linear(inputs=, mask_bits=)`, csrc/edge_wgrad16.hip
through `ops.edge_weight_grad(inputs=)`, the autograd node through `scatter.edge_linear(inputs=)`, and the GGNN layer's
edge-form training branch under `ptgnn_amd.matrix_inputs(dt, edge_training=True)`.

Reference: float64 on the ROUNDED operands -- the forward and the weight gradient round (x.float() * scale32) under the
mask unpacked on the host from `ops.dropout_bitmask` of the same (p, seed); bar: C.bar for the forward and the input
gradient, T.floored_bar for the weight gradient and d_x, which sum over rows (tests/edge_training_cases.py).  Every numeric
test first asserts, from the two float64 references alone, that rounding moves the result by at least 20 bars
(tests/test_edge_training_cpu.py checks the same on the CPU under an arbitrary Bernoulli mask), and then that the kernel's
result is within one bar of the rounded reference and at least `gap - bar` from the exact one."""
import ctypes

import pytest
import torch

import edge_training_cases as E
import half_cases as C
import half_training_cases as T

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
SEED = E.SEED
HALF_FAMILIES = ("half_linear", "half_gru", "half_wgrad", "half_gru_train", "half_linear_add", "edge16", "edge16_shared")


def _launches(fn):
    """(result of fn, {family: launches it made}) over the GEMM families, every half family and the new ones."""
    from ptgnn_amd import ops
    before = ops.launch_counts(half=True, edge16=True, half_training=True, edge16_training=True)
    out = fn()
    return out, ops.launches_since(before)


def _cuda_adj(adj):
    return [(s.cuda(), d.cuda()) for s, d in adj]


def _identity(counts):
    """The identity index of the input gradient: row r of the incoming gradient is message row r."""
    off, out = 0, []
    for c in counts:
        i = torch.arange(off, off + c, dtype=torch.int64, device="cuda")
        out.append((i, i))
        off += c
    return out


def _entry(x, adj, w16, dt, out, mode, p, bits):
    """ptgnn_amd_edge_masked_linear16 into `out`, a view with a row stride of its own."""
    from ptgnn_amd import _lib, ops
    lib = _lib.load()
    n_types = len(adj)
    Ptr, Cnt = ctypes.c_void_p * n_types, ctypes.c_int64 * n_types
    srcs = [s.contiguous() for s, _ in adj]
    sp = Ptr(*[s.data_ptr() if s.numel() else None for s in srcs])
    cn = Cnt(*[int(s.shape[0]) for s in srcs])
    assert x.stride(1) == 1 and out.stride(1) == 1 and w16.is_contiguous()
    rc = lib.ptgnn_amd_edge_masked_linear16(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1],
                                            ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(cn, ctypes.c_void_p),
                                            w16.data_ptr(), n_types, out.shape[1], ops.HALF_IDS[dt], out.data_ptr(),
                                            out.stride(0), mode, p, bits.data_ptr() if bits is not None else None,
                                            torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ptgnn_amd_edge_masked_linear16")
    torch.cuda.synchronize()
    return out


def _nan_outside(view, left, right):
    """Everything of the NaN-padded buffer around `view` (T.strided_nan) is still NaN."""
    base = view._base
    cols = view.shape[1]
    return bool(base[:, :left].isnan().all()) and bool(base[:, left + cols:].isnan().all()) and base.shape[1] == left + cols + right


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward (mode 1) and input gradient (mode 2) against float64, into a NaN-padded strided view
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_masked_forward_and_input_gradient_against_float64(dt, h, m):
    from ptgnn_amd import ops
    x, ws, adj, g = E.edge_case(h, m)
    counts = [int(s.shape[0]) for s, _ in adj]
    n_edges = sum(counts)
    cadj = _cuda_adj(adj)
    bits = ops.dropout_bitmask(n_edges, h, E.P, SEED, "cuda")
    keep = E.unpack(bits, h)
    assert 0.6 < float(keep.float().mean()) < 0.9
    assert torch.equal(keep, E.hash_keep(n_edges, h, E.P, SEED))                 # the mask the CPU suite checked the case under
    refs = E.references(x, ws, adj, g, keep, E.P, dt)
    xg, gg = x.cuda(), g.cuda()
    wsg = [w.cuda() for w in ws]
    w16 = torch.stack(wsg).to(dt).contiguous()                                   # [T, M, H]
    wt16 = torch.stack(wsg).transpose(1, 2).contiguous().to(dt).contiguous()      # [T, H, M]

    out = T.strided_nan(torch.zeros(n_edges, m, device="cuda"), 4, 8)
    got, since = _launches(lambda: _entry(xg, cadj, w16, dt, out, 1, E.P, bits))
    assert since == {"edge16_masked": 1}, since
    assert _nan_outside(out, 4, 8) and not bool(got.isnan().any())
    T.check(got, *refs["msg"], f"{C.IDS[dt]} ({h}, {m}) forward")
    via_ops, since = _launches(lambda: ops.edge_linear(xg, cadj, wsg, False, dropout=(1, E.P, SEED), mask_bits=bits,
                                                       inputs=dt))
    assert since == {"edge16_masked": 1} and torch.equal(via_ops, got), since
    given = ops.edge_linear(xg, cadj, wsg, False, dropout=(1, E.P, SEED), mask_bits=bits, inputs=dt, rounded=w16)
    assert torch.equal(given, got)

    out2 = T.strided_nan(torch.zeros(n_edges, h, device="cuda"), 8, 4)
    got2, since = _launches(lambda: _entry(gg, _identity(counts), wt16, dt, out2, 2, E.P, bits))
    assert since == {"edge16_masked": 1}, since
    assert _nan_outside(out2, 8, 4) and not bool(got2.isnan().any())
    T.check(got2, *refs["g_in"], f"{C.IDS[dt]} ({h}, {m}) input gradient")
    assert bool((got2.cpu()[~keep] == 0).all())                                  # a dropped element is exactly zero
    via_ops, since = _launches(lambda: ops.edge_linear(gg, _identity(counts), [w.t().contiguous() for w in wsg], False,
                                                       dropout=(2, E.P, SEED), mask_bits=bits, inputs=dt))
    assert since == {"edge16_masked": 1} and torch.equal(via_ops, got2), since


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact integer data, p = 0.5 (scale exactly 2): the three launches are exact and bit-equal to the fp32 masked entries
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_integer_case_is_exact_and_bit_equal_to_the_fp32_masked_entries(dt, h, m):
    from ptgnn_amd import ops
    x, ws, adj, g = E.integer_case(h, m, E.COUNTS, 9500 + h + m)
    counts = list(E.COUNTS)
    n_edges = sum(counts)
    cadj, ident = _cuda_adj(adj), _identity(counts)
    bits = ops.dropout_bitmask(n_edges, h, 0.5, SEED, "cuda")
    keep = E.unpack(bits, h)
    assert E.scale32(0.5) == 2.0
    xg, gg = x.cuda(), g.cuda()
    wsg = [w.cuda() for w in ws]
    wtg = [w.t().contiguous() for w in wsg]

    got, since = _launches(lambda: ops.edge_linear(xg, cadj, wsg, False, dropout=(1, 0.5, SEED), mask_bits=bits, inputs=dt))
    assert since == {"edge16_masked": 1}, since
    assert torch.equal(got.cpu(), E.forward64(x, adj, ws, keep, 0.5).float())
    assert torch.equal(got, ops.edge_linear(xg, cadj, wsg, False, dropout=(1, 0.5, SEED), mask_bits=bits))

    got, since = _launches(lambda: ops.edge_linear(gg, ident, wtg, False, dropout=(2, 0.5, SEED), mask_bits=bits, inputs=dt))
    assert since == {"edge16_masked": 1}, since
    assert torch.equal(got.cpu(), E.input_grad64(g, counts, ws, keep, 0.5).float())
    assert torch.equal(got, ops.edge_linear(gg, ident, wtg, False, dropout=(2, 0.5, SEED), mask_bits=bits))

    got, since = _launches(lambda: ops.edge_weight_grad(xg, cadj, gg, False, 0.5, SEED, mask_bits=bits, inputs=dt))
    assert since == {"edge_wgrad16": 1}, since
    assert torch.equal(got.cpu(), E.wgrad64(x, adj, g, keep, 0.5).float())
    assert torch.equal(got, ops.edge_weight_grad(xg, cadj, gg, False, 0.5, SEED, mask_bits=bits))
    assert not bool(got[0].any())                                                # the empty type


# ---------------------------------------------------------------------------------------------------------------------
# 3. weight gradient against float64: two chunks with a ragged panel, an empty type, a single edge
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("h,m", E.WGRAD_SHAPES)
def test_weight_gradient_against_float64(dt, h, m):
    from ptgnn_amd import ops
    chunk = ops.edge_wgrad16_chunk_edges(1, 4, m, h)
    counts = E.wgrad_counts(chunk)
    assert chunk == E.MIN_CHUNK and ops.edge_wgrad16_chunk_edges(sum(counts), len(counts), m, h) == chunk
    x, ws, adj, g = E.wgrad_case(h, m, chunk)
    n_edges = sum(counts)
    cadj = _cuda_adj(adj)
    bits = ops.dropout_bitmask(n_edges, h, E.P, SEED, "cuda")
    keep = E.unpack(bits, h)
    xg = T.strided_nan(x.cuda(), 4, 4)
    gg = T.strided_nan(g.cuda(), 8, 0)
    for mask, kp, p in ((bits, keep, E.P), (None, None, 0.0)):
        rounded, exact, bar = E.references(x, ws, adj, g, kp, p, dt)["d_w"]
        got, since = _launches(lambda: ops.edge_weight_grad(xg, cadj, gg, False, p, SEED, mask_bits=mask, inputs=dt))
        assert since == {"edge_wgrad16": 1}, since
        assert got.shape == (len(counts), m, h)
        T.check(got, rounded, exact, bar, f"{C.IDS[dt]} ({h}, {m}) weight gradient{'' if mask is None else ', masked'}")
        assert not bool(got[1].any())                                            # the empty type's row: exactly zero
        again = ops.edge_weight_grad(xg, cadj, gg, False, p, SEED, mask_bits=mask, inputs=dt)
        assert torch.equal(again, got)                                           # two calls, the same bits
    # a type alone in its chunk is written in place: the same bits as the fp32-free restatement on one type at a time
    one = ops.edge_weight_grad(xg, [cadj[3], cadj[1]], gg[counts[0] + counts[1] + counts[2]:], False, 0.0, SEED, inputs=dt)
    assert torch.equal(one[0], got[3]) and not bool(one[1].any())


# ---------------------------------------------------------------------------------------------------------------------
# 4. without a mask the entry is the unmasked launch, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_entry_without_a_mask_has_the_bits_of_the_unmasked_launch(dt, h, m):
    from ptgnn_amd import ops
    x, ws, adj, _ = E.edge_case(h, m)
    cadj = _cuda_adj(adj)
    xg, wsg = x.cuda(), [w.cuda() for w in ws]
    w16 = torch.stack(wsg).to(dt).contiguous()
    want, since = _launches(lambda: ops.edge_linear(xg, cadj, wsg, False, inputs=dt))
    assert since == {"edge16": 1}, since
    n_edges = want.shape[0]
    bits = ops.dropout_bitmask(n_edges, h, E.P, SEED, "cuda")
    for mode, p, mask in ((1, E.P, None), (0, E.P, bits), (1, 0.0, bits), (2, E.P, None)):
        out = T.strided_nan(torch.zeros(n_edges, m, device="cuda"), 4, 4)
        got, since = _launches(lambda: _entry(xg, cadj, w16, dt, out, mode, p, mask))
        assert since == {"edge16": 1} and torch.equal(got, want), (mode, p, since)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the autograd node: scatter.edge_linear(..., inputs=dt), forward and backward
# ---------------------------------------------------------------------------------------------------------------------
def _node(x, plan, w_stack, p, go, **kw):
    from ptgnn_amd import scatter
    x = x.detach().clone().requires_grad_(True)
    w = w_stack.detach().clone().requires_grad_(True)
    msg, since_f = _launches(lambda: scatter.edge_linear(x, plan, w, False, p, SEED, **kw))
    _, since_b = _launches(lambda: msg.backward(go))
    return msg.detach(), x.grad, w.grad, since_f, since_b


@DTYPES
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_autograd_node_forward_and_backward(dt, h, m):
    from ptgnn_amd import ops
    x, ws, adj, g = E.edge_case(h, m)
    n_edges = g.shape[0]
    cadj = _cuda_adj(adj)
    ops.clear_plan_cache()
    plan = ops.plan_for(cadj, E.N)
    keep = E.unpack(ops.dropout_bitmask(n_edges, h, E.P, SEED, "cuda"), h)
    refs = E.references(x, ws, adj, g, keep, E.P, dt)
    xg, gg, w_stack = x.cuda(), g.cuda(), torch.stack([w.cuda() for w in ws])

    msg, d_x, d_w, since_f, since_b = _node(xg, plan, w_stack, E.P, gg, inputs=dt)
    assert since_f.get("edge16_masked") == 1 and since_b.get("edge16_masked") == 1 and since_b.get("edge_wgrad16") == 1
    fp32 = E.FP32_EDGE_FAMILIES + E.FP32_WGRAD_FAMILIES
    assert not [f for f in fp32 if f in since_f or f in since_b], (since_f, since_b)
    assert msg.dtype == d_x.dtype == d_w.dtype == torch.float32
    what = f"{C.IDS[dt]} ({h}, {m})"
    T.check(msg, *refs["msg"], what + " msg")
    T.check(d_x, *refs["d_x"], what + " d_x")
    T.check(d_w, *refs["d_w"], what + " d_w")
    again = _node(xg, plan, w_stack, E.P, gg, inputs=dt)
    assert all(torch.equal(a, b) for a, b in zip(again[:3], (msg, d_x, d_w)))   # deterministic

    today = _node(xg, plan, w_stack, E.P, gg)                                   # without the keyword: today's call
    for kw in ({"inputs": None}, {"inputs": torch.float32}):
        got = _node(xg, plan, w_stack, E.P, gg, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], today[:3])), kw
        assert not [f for f in E.MASKED_FAMILIES if f in got[3] or f in got[4]], kw
    assert not torch.equal(today[0], msg)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the GGNN layer's edge-form training branch
# ---------------------------------------------------------------------------------------------------------------------
def _layer_case(dropout, h=64, types=3, counts=(300, 200, 100)):
    from ptgnn_amd import layers as L
    torch.manual_seed(9600)
    layer = L.GatedMessagePassingLayer(h, h, types, "sum", dropout_rate=dropout)
    x = torch.randn(200, h, generator=torch.Generator().manual_seed(9601))
    adj = C.random_adjacency(200, counts, 9602)
    return layer.cuda(), x.cuda(), _cuda_adj(adj)


def _step(layer, x, adj):
    """One seeded training step: (output, gradients of every parameter and of the states, launches of the forward,
    launches of the backward)."""
    from ptgnn_amd import ops
    ops.clear_plan_cache()
    layer.zero_grad()
    torch.manual_seed(9603)
    x = x.detach().clone().requires_grad_(True)
    feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    out, since_f = _launches(lambda: layer(x, adj, None, {}, {}, feats))
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(9604)).to(out.device, out.dtype)
    _, since_b = _launches(lambda: out.backward(go))
    return out.detach(), [p.grad.clone() for p in layer.parameters()] + [x.grad.clone()], since_f, since_b


def _count(since, families):
    return sum(since.get(f, 0) for f in families)


@DTYPES
def test_layer_with_dropout_takes_the_16_bit_edge_node_under_the_flag(dt):
    import ptgnn_amd
    layer, x, adj = _layer_case(0.2)
    layer.train()
    default, default_grads, def_f, def_b = _step(layer, x, adj)
    assert not [f for f in E.MASKED_FAMILIES + HALF_FAMILIES if f in def_f or f in def_b], (def_f, def_b)
    assert _count(def_f, E.FP32_EDGE_FAMILIES) == 1 and _count(def_b, E.FP32_EDGE_FAMILIES) == 1
    with ptgnn_amd.matrix_inputs(dt, edge_training=True):
        got, grads, since_f, since_b = _step(layer, x, adj)
        again, again_grads, _, _ = _step(layer, x, adj)
    assert ptgnn_amd.get_matrix_inputs() is torch.float32
    assert since_f.get("edge16_masked") == 1 and "edge_wgrad16" not in since_f, since_f
    assert since_b.get("edge16_masked") == 1 and since_b.get("edge_wgrad16") == 1, since_b
    assert _count(since_f, E.FP32_EDGE_FAMILIES) == 0 and _count(since_b, E.FP32_EDGE_FAMILIES) == 0, (since_f, since_b)
    # the fp32 weight-gradient families serve the GRU node too: the edge node's one launch of them is gone
    assert _count(since_b, E.FP32_WGRAD_FAMILIES) == _count(def_b, E.FP32_WGRAD_FAMILIES) - 1, (since_b, def_b)
    assert not [f for f in HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)   # the GRU node: still fp32
    assert torch.equal(again, got) and all(torch.equal(p, q) for p, q in zip(again_grads, grads))   # two seeded steps
    assert not torch.equal(got, default)
    # A sanity bound on the whole step (the stage tests above hold each GEMM to its bar): the same seed draws the same
    # mask, so the two steps differ by the roundings alone -- a gradient passes through at most two rounded GEMMs, each
    # moving its result by at most 2 u relative to the result's scale (u = 2^-9 for bf16, 2^-12 for fp16, both operands
    # rounded), and through the gate math's derivatives, which are at most 1: 4 u, with a factor 4 of headroom for the
    # scales of intermediate results against the final one.
    u = 2.0 ** -9 if dt is torch.bfloat16 else 2.0 ** -12
    for p, q in zip(grads, default_grads):
        moved = float((p - q).abs().max())
        print(f"  gradient {tuple(q.shape)}: moved {moved:.3e}, scale {float(q.abs().max()):.3e}")
        assert moved <= 16 * u * max(1.0, float(q.abs().max()))
    with ptgnn_amd.matrix_inputs(torch.float32, edge_training=True):            # accepted, means fp32
        same, same_grads, f32_f, f32_b = _step(layer, x, adj)
    assert torch.equal(same, default) and all(torch.equal(p, q) for p, q in zip(same_grads, default_grads))
    assert not [f for f in E.MASKED_FAMILIES if f in f32_f or f in f32_b]


@DTYPES
def test_layer_without_the_keyword_keeps_its_launches_and_bits(dt):
    import ptgnn_amd
    layer, x, adj = _layer_case(0.2)
    layer.train()
    default, default_grads, _, _ = _step(layer, x, adj)
    with ptgnn_amd.matrix_inputs(dt):                                          # the dtype alone: fp32 in training
        got, grads, since_f, since_b = _step(layer, x, adj)
    assert torch.equal(got, default) and all(torch.equal(p, q) for p, q in zip(grads, default_grads))
    with ptgnn_amd.matrix_inputs(dt, training=True):                            # the GRU node rounds, the edge node does not
        tr, tr_grads, tr_f, tr_b = _step(layer, x, adj)
    with ptgnn_amd.matrix_inputs(dt, edge_gemm=True, training=True):
        both, both_grads, both_f, both_b = _step(layer, x, adj)
    for since_f, since_b in ((tr_f, tr_b), (both_f, both_b)):
        assert not [f for f in E.MASKED_FAMILIES + ("edge16", "edge16_shared") if f in since_f or f in since_b]
        assert since_f.get("half_gru_train") == 1 and _count(since_f, E.FP32_EDGE_FAMILIES) == 1, since_f
        assert _count(since_b, E.FP32_EDGE_FAMILIES) == 1 and _count(since_b, E.FP32_WGRAD_FAMILIES) == 1, since_b
        assert since_b.get("half_wgrad") == 2 and since_b.get("half_linear_add") == 1 and since_b.get("half_linear") == 1
    assert (tr_f, tr_b) == (both_f, both_b)
    assert torch.equal(both, tr) and all(torch.equal(p, q) for p, q in zip(both_grads, tr_grads))
    with ptgnn_amd.matrix_inputs(dt, training=True, edge_training=True):        # and the two flags together: both nodes
        _, _, since_f, since_b = _step(layer, x, adj)
    assert since_f.get("edge16_masked") == 1 and since_f.get("half_gru_train") == 1, since_f
    assert since_b.get("edge16_masked") == 1 and since_b.get("edge_wgrad16") == 1 and since_b.get("half_wgrad") == 2, since_b
    assert _count(since_b, E.FP32_WGRAD_FAMILIES) == 0 and _count(since_b, E.FP32_EDGE_FAMILIES) == 0, since_b


@DTYPES
def test_training_forward_without_dropout_has_the_bits_of_the_inference_edge_form(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    layer, x, adj = _layer_case(0.0, types=8, counts=(100, 90, 80, 70, 0, 60, 33, 1))
    assert L._prefer_edge_path(434, 200, 8, 64, 64)                             # an edge-form batch
    layer.train()
    with ptgnn_amd.matrix_inputs(dt, training=True, edge_training=True):
        got, _, since_f, since_b = _step(layer, x, adj)
    assert since_f.get("edge16") == 1 and since_f.get("half_gru_train") == 1, since_f      # no mask: the unmasked launch
    assert since_b.get("edge16") == 1 and since_b.get("edge_wgrad16") == 1, since_b
    assert _count(since_f, E.FP32_EDGE_FAMILIES) == 0 and _count(since_b, E.FP32_EDGE_FAMILIES + E.FP32_WGRAD_FAMILIES) == 0
    layer.eval()
    feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt, edge_gemm=True):
        inference = layer(x, adj, None, {}, {}, feats)
    assert torch.equal(got, inference)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a width the 16-bit kernels do not take runs fp32, silently
# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_width_runs_fp32_silently_under_the_flag():
    import ptgnn_amd
    layer, x, adj = _layer_case(0.2, h=48)
    layer.train()
    default, default_grads, _, _ = _step(layer, x, adj)
    # this width takes `_general_messages`, whose index_select backward adds with atomics in torch: the state gradient of
    # that route is not repeatable run to run with no setting at all, so "the same bits" is asked of everything that is
    repeat, repeat_grads, _, _ = _step(layer, x, adj)
    assert torch.equal(repeat, default)
    repeatable = [torch.equal(p, q) for p, q in zip(repeat_grads, default_grads)]
    print(f"  repeatable without any setting: {repeatable}")
    repeatable[-1] = False                                                      # the state gradient: never relied on
    for dt in C.HALF:
        with ptgnn_amd.matrix_inputs(dt, edge_training=True):
            got, grads, since_f, since_b = _step(layer, x, adj)
        assert not [f for f in E.MASKED_FAMILIES + HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
        assert torch.equal(got, default)
        for p, q, same in zip(grads, default_grads, repeatable):
            if same:
                assert torch.equal(p, q)
            else:                                                               # fp32 sums in another order: ulps, not 2^-9
                assert float((p - q).abs().max()) <= 1e-5 * max(1.0, float(q.abs().max()))
