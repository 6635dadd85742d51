"""The opt-in 16-bit matrix inputs of the GGNN training step on the MI355X: csrc/wgrad16.hip through
`ops.half_linear_weight_grad`, the training forms of csrc/half_gemm.hip through `ops.gru_cell_train` / `ops.linear_add`
(`inputs=`), the 16-bit autograd nodes of ptgnn_amd/dense.py stage by stage, and the GGNN layer's training routes under
`ptgnn_amd.matrix_inputs(dt, training=True)`.

Reference: float64 on the ROUNDED operands; bar: TOL * max(1, |want|inf) with the floor of
tests/half_training_cases.py for sums over every row.  Every numeric test first asserts, from the two float64
references alone, that rounding moves the result by at least 20 bars, and then that the kernel's result is within one bar
of the rounded reference and at least `gap - bar` from the exact one.  Where a node rounds a value it computed (the
gate-math backward's d_gi, d_gh), the reference takes exactly the captured fp32 operand (tests/half_cases.py says why)."""
import pytest
import torch

import half_cases as C
import half_training_cases as T

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
HALF_FAMILIES = ("half_linear", "half_gru") + T.TRAIN_FAMILIES


def _launches(fn):
    """(result of fn, {family: launches it made}) over the fp32 GEMM families and every half family."""
    from ptgnn_amd import ops
    before = ops.launch_counts(half=True, half_training=True)
    out = fn()
    return out, ops.launches_since(before)


def _cuda(*ts):
    return [t.cuda() if t is not None else None for t in ts]


def _chunk(k, n_out):
    """Rows per workgroup partial at the tests' row counts, and the row count with two whole partials and a short one."""
    from ptgnn_amd import ops
    chunk = ops.half_wgrad_chunk_rows(1, n_out, k)
    rows = 2 * chunk + 17
    assert chunk > 0 and ops.half_wgrad_chunk_rows(rows, n_out, k) == chunk
    return chunk, rows


# ---------------------------------------------------------------------------------------------------------------------
# 1. weight gradient, exact integer data: the transposed fragments, row tails, several partials, strided views
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("k,n_out", T.WGRAD_SHAPES)
def test_weight_grad_is_exact_on_integer_data(dt, k, n_out):
    from ptgnn_amd import ops
    _, many = _chunk(k, n_out)
    x_all, g_all = T.wgrad_integer_case(many, k, n_out, 8000 + k + n_out)
    xg_all, gg_all = _cuda(x_all, g_all)
    for rows in (1, 15, 16, 17, 31, 33, 129, many):
        want_w, want_b = T.wgrad_exact(x_all[:rows], g_all[:rows])
        for strided in (False, True):
            if strided:
                xg, gg = T.strided_nan(xg_all[:rows], 4, 4), T.strided_nan(gg_all[:rows], n_out + 4, 0)
            else:
                xg, gg = xg_all[:rows], gg_all[:rows]
            what = (C.IDS[dt], rows, k, n_out, strided)
            (gw, gb), since = _launches(lambda: ops.half_linear_weight_grad(xg, gg, dt, want_bias=True))
            assert since == {"half_wgrad": 1}, (what, since)
            assert torch.equal(gw.cpu(), want_w) and torch.equal(gb.cpu(), want_b), what
            alone, since = _launches(lambda: ops.half_linear_weight_grad(xg, gg, dt))
            assert since == {"half_wgrad": 1}, (what, since)
            assert torch.equal(alone.cpu(), want_w), what
    gw, gb = ops.half_linear_weight_grad(xg_all[:0], gg_all[:0], dt, want_bias=True)          # no rows: zeros
    assert gw.shape == (n_out, k) and not bool(gw.any()) and gb.shape == (n_out,) and not bool(gb.any())


def test_weight_grad_outside_the_kernel_runs_fp32_silently():
    from ptgnn_amd import ops
    gen = torch.Generator().manual_seed(8100)
    x, g = torch.randn(50, 36, generator=gen).cuda(), torch.randn(50, 64, generator=gen).cuda()    # k % 32 != 0
    got, since = _launches(lambda: ops.half_linear_weight_grad(x, g, torch.bfloat16))
    assert not [f for f in HALF_FAMILIES if f in since] and since, since
    assert torch.equal(got, ops.linear_weight_grad(x, g))
    x32, g32 = torch.randn(50, 32, generator=gen).cuda(), torch.randn(50, 64, generator=gen).cuda()
    got, since = _launches(lambda: ops.half_linear_weight_grad(x32, g32, torch.float32))      # float32: the fp32 kernel
    assert not [f for f in HALF_FAMILIES if f in since] and torch.equal(got, ops.linear_weight_grad(x32, g32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. weight gradient, random data against float64 on the rounded operands
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("k,n_out", [(128, 384), (64, 96)])
@pytest.mark.parametrize("many", [False, True], ids=["rows300", "partials"])
def test_weight_grad_matches_float64_on_the_rounded_operands(dt, k, n_out, many):
    from ptgnn_amd import ops
    rows = _chunk(k, n_out)[1] if many else 300
    x, g = T.wgrad_random_case(rows, k, n_out, 7000)
    xg, gg = _cuda(x, g)
    (gw, gb), since = _launches(lambda: ops.half_linear_weight_grad(xg, gg, dt, want_bias=True))
    assert since == {"half_wgrad": 1}, since
    T.check(gw, T.wgrad64(x, g, dt), T.wgrad64(x, g), T.wgrad_bar(x, g, dt),
            f"weight grad {C.IDS[dt]} rows={rows} k={k} n_out={n_out}")
    want_b = g.double().sum(dim=0)                                    # the UNROUNDED gradient
    e_b = C.err(gb, want_b)
    print(f"  bias grad: |got - float64| {e_b:.3e} (bar {T.grad_bar(want_b):.3e})")
    assert e_b <= T.grad_bar(want_b)
    assert C.err(C.rnd64(g, dt).sum(dim=0), want_b) > T.grad_bar(want_b)        # ... which rounding would have missed
    again_w, again_b = ops.half_linear_weight_grad(xg, gg, dt, want_bias=True)
    assert torch.equal(again_w, gw) and torch.equal(again_b, gb)
    assert torch.equal(ops.half_linear_weight_grad(xg, gg, dt), gw)             # the bias output changes nothing


# ---------------------------------------------------------------------------------------------------------------------
# 3. the training form of the 16-bit GRU cell
# ---------------------------------------------------------------------------------------------------------------------
GRU_SEEDS = {(64, 64): 7100, (128, 128): 7100, (96, 96): 7101}       # found on the CPU: >= 27 bars at every row count


@pytest.fixture(scope="module")
def gru_cases():
    return {key: C.gru_case(300, *key, seed) for key, seed in GRU_SEEDS.items()}


@DTYPES
@pytest.mark.parametrize("m,hd", list(GRU_SEEDS))
@pytest.mark.parametrize("rows", [1, 33, 300])
def test_gru_training_cell_has_the_inference_bits_and_the_float64_gates(gru_cases, dt, m, hd, rows):
    from ptgnn_amd import ops
    a, h, *params = gru_cases[(m, hd)]
    a, h = a[:rows], h[:rows]
    ag, hg, *pg = _cuda(a, h, *params)
    (out, gates), since = _launches(lambda: ops.gru_cell_train(ag, hg, *pg, inputs=dt))
    assert since == {"half_gru_train": 1}, since
    assert torch.equal(out, ops.gru_cell(ag, hg, *pg, inputs=dt))
    rounded = T.gates64(a, h, *params, dt=dt)
    T.check(gates, rounded, T.gates64(a, h, *params), C.bar(rounded), f"gates {C.IDS[dt]} rows={rows} m={m} hd={hd}")
    given = ops.gru_cell_train(ag, hg, *pg, inputs=dt, rounded=(pg[0].to(dt), pg[1].to(dt)))
    assert torch.equal(given[0], out) and torch.equal(given[1], gates)
    fp32 = ops.gru_cell_train(ag, hg, *pg)                                       # without the keyword: today's cell
    assert torch.equal(fp32[0], ops.gru_cell_train(ag, hg, *pg, inputs=torch.float32)[0])
    assert not torch.equal(fp32[0], out)


def test_gru_training_cell_writes_nothing_past_its_rows():
    from ptgnn_amd import _lib, ops
    dt = torch.bfloat16
    a, h, *params = C.gru_case(45, 128, 128, 7102)
    ag, hg, *pg = _cuda(a, h, *params)
    out, gates = ops.gru_cell_train(ag, hg, *pg, inputs=dt)
    lib = _lib.load()
    obuf = torch.full((47, 128), float("nan"), device="cuda")
    gbuf = torch.full((47, 512), float("nan"), device="cuda")
    w16 = [pg[0].to(dt).contiguous(), pg[1].to(dt).contiguous()]
    rc = lib.ptgnn_amd_gru_cell_train16(ag.data_ptr(), 128, hg.data_ptr(), 128, w16[0].data_ptr(), w16[1].data_ptr(),
                                        pg[2].data_ptr(), pg[3].data_ptr(), 45, 128, 128, ops.HALF_IDS[dt],
                                        obuf.data_ptr(), 128, gbuf.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(obuf[:45], out) and torch.equal(gbuf[:45], gates)
    assert bool(obuf[45:].isnan().all()) and bool(gbuf[45:].isnan().all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the 16-bit Linear with an fp32 addend
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_linear_add_is_the_half_linear_plus_the_addend(dt):
    from ptgnn_amd import ops
    gen = torch.Generator().manual_seed(8400)
    for rows, k, n_out in ((300, 128, 384), (33, 96, 160)):
        x, w, b = torch.randn(rows, k, generator=gen), C.xavier(n_out, k, gen), torch.randn(n_out, generator=gen) * 0.1
        addend = torch.randn(rows, n_out, generator=gen)
        xg, wg, bg, addg = _cuda(x, w, b, addend)
        for bias, act in ((None, None), (bg, "tanh")):
            got, since = _launches(lambda: ops.linear_add(xg, wg, addg, bias, act=act, inputs=dt))
            assert since == {"half_linear_add": 1}, since
            want = ops.linear(xg, wg, bias, act=act, inputs=dt).double() + addg.double()
            # one fp32 rounding of the sum per element
            assert bool(((got.double() - want).abs() <= 2.0 ** -24 * want.abs() + 1e-45).all()), (rows, k, n_out, act)
        view = T.strided_nan(addg, 4, 3)                               # the addend has its own leading dimension
        assert torch.equal(ops.linear_add(xg, wg, view, inputs=dt), ops.linear_add(xg, wg, addg, inputs=dt))
    x, w, b = C.integer_case(129, 64, 96, 8401)
    addend = torch.randint(-50, 51, (129, 96), generator=gen).float()
    xg, wg, bg, addg = _cuda(x, w, b, addend)
    for rows in (1, 33, 129):
        got = ops.linear_add(xg[:rows], wg, addg[:rows], bg, inputs=dt)
        assert torch.equal(got.cpu(), x[:rows] @ w.t() + b + addend[:rows]), rows
    x30 = torch.randn(20, 30, generator=gen).cuda()                       # outside the kernel: fp32, silently
    w30, add30 = torch.randn(64, 30, generator=gen).cuda(), torch.randn(20, 64, generator=gen).cuda()
    got, since = _launches(lambda: ops.linear_add(x30, w30, add30, inputs=dt))
    assert not [f for f in HALF_FAMILIES if f in since], since
    assert torch.equal(got, ops.linear_add(x30, w30, add30))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the autograd nodes, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
def _linear_node_case(rows, k, n_out, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, k, generator=gen), C.xavier(n_out, k, gen), torch.randn(n_out, generator=gen) * 0.1,
            torch.randn(rows, n_out, generator=gen))


@DTYPES
def test_linear_node_rounds_every_gemm_and_nothing_else(dt):
    from ptgnn_amd import dense
    x, w, b, g = _linear_node_case(300, 64, 96, 7500)
    xg, wg, bg, gg = _cuda(x, w, b, g)
    for t in (xg, wg, bg):
        t.requires_grad_(True)
    dense.clear_transposed_cache()
    y, since = _launches(lambda: dense.linear(xg, wg, bg, inputs=dt))
    assert since == {"half_linear": 1}, since
    rounded = C.linear64(x, w, b, None, dt)
    T.check(y, rounded, C.linear64(x, w, b), C.bar(rounded), f"linear node forward {C.IDS[dt]}")
    _, since = _launches(lambda: y.backward(gg))
    assert since == {"half_linear": 1, "half_wgrad": 1}, since           # no fp32 GEMM family
    T.check(xg.grad, C.rnd64(g, dt) @ C.rnd64(w, dt), g.double() @ w.double(),
            T.matmul_bar(g, w.t().contiguous(), dt), f"linear node d_x {C.IDS[dt]}")
    T.check(wg.grad, T.wgrad64(x, g, dt), T.wgrad64(x, g), T.wgrad_bar(x, g, dt), f"linear node d_W {C.IDS[dt]}")
    want_b = g.double().sum(dim=0)
    assert C.err(bg.grad, want_b) <= T.grad_bar(want_b)
    # the default node is today's: same bits as without the keyword, fp32 families only
    x0, w0, b0 = (t.detach().clone().requires_grad_(True) for t in (xg, wg, bg))
    x1, w1, b1 = (t.detach().clone().requires_grad_(True) for t in (xg, wg, bg))
    _, since = _launches(lambda: dense.linear(x0, w0, b0).backward(gg))
    assert not [f for f in HALF_FAMILIES if f in since], since
    dense.linear(x1, w1, b1, inputs=torch.float32).backward(gg)
    assert all(torch.equal(p.grad, q.grad) for p, q in ((x0, x1), (w0, w1), (b0, b1)))


def test_linear_node_at_width_30_runs_the_fp32_kernels_alone():
    from ptgnn_amd import dense
    x, w, b, g = _linear_node_case(100, 30, 30, 7501)
    xg, wg, bg, gg = _cuda(x, w, b, g)
    ref = [t.detach().clone().requires_grad_(True) for t in (xg, wg, bg)]
    for t in (xg, wg, bg):
        t.requires_grad_(True)
    y, since_f = _launches(lambda: dense.linear(xg, wg, bg, inputs=torch.bfloat16))
    _, since_b = _launches(lambda: y.backward(gg))
    assert since_f and since_b and not [f for f in HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
    y0 = dense.linear(*ref)
    y0.backward(gg)
    assert torch.equal(y, y0) and all(torch.equal(p.grad, q.grad) for p, q in zip((xg, wg, bg), ref))


def _gru_node_case(m, hd, seed, rows=300):
    """C.gru_case with the update gate's input bias shifted by -4 (z around 0.02): the direct term g z of d_h is then
    small beside rnd(d_gh) rnd(W_hh), so that GEMM's rounding is visible on the scale of their sum (with z around 0.5
    the sum's bar hides it for fp16: 15 bars on the CPU for every seed tried; with the shift 27 and more at this seed,
    from a CPU restatement of the captured operands)."""
    a, h, w_ih, w_hh, b_ih, b_hh = C.gru_case(rows, m, hd, seed)
    b_ih = b_ih.clone()
    b_ih[hd:2 * hd] -= 4.0
    go = torch.randn(rows, hd, generator=torch.Generator().manual_seed(seed + 50000))
    return a, h, w_ih, w_hh, b_ih, b_hh, go


GRU_NODE_SEEDS = {(64, 64): 7700, (128, 128): 7700, (96, 96): 7700}


@DTYPES
@pytest.mark.parametrize("m,hd", list(GRU_NODE_SEEDS))
def test_gru_node_rounds_every_gemm_of_its_backward(monkeypatch, dt, m, hd):
    from ptgnn_amd import dense, ops
    a, h, w_ih, w_hh, b_ih, b_hh, go = _gru_node_case(m, hd, GRU_NODE_SEEDS[(m, hd)])
    ts = _cuda(a, h, w_ih, w_hh, b_ih, b_hh)
    for t in ts:
        t.requires_grad_(True)
    gog = go.cuda()
    dense.clear_transposed_cache()
    out, since = _launches(lambda: dense.gru_cell_weights(*ts, inputs=dt))
    assert since == {"half_gru_train": 1}, since
    assert torch.equal(out, ops.gru_cell(*[t.detach() for t in ts], inputs=dt))
    with C.captured(monkeypatch, ops, "gru_gates_backward") as seen:
        _, since = _launches(lambda: out.backward(gog))
    assert since == {"half_linear": 1, "half_linear_add": 1, "half_wgrad": 2}, since       # no fp32 GEMM family
    assert len(seen) == 1
    d_gi, d_gh, d_h = (t.detach().cpu() for t in seen[0])
    what = f"gru node {C.IDS[dt]} m={m} hd={hd}"
    T.check(ts[0].grad, C.rnd64(d_gi, dt) @ C.rnd64(w_ih, dt), d_gi.double() @ w_ih.double(),
            T.matmul_bar(d_gi, w_ih.t().contiguous(), dt), what + " d_a")
    T.check(ts[1].grad, C.rnd64(d_gh, dt) @ C.rnd64(w_hh, dt) + d_h.double(), d_gh.double() @ w_hh.double() + d_h.double(),
            T.matmul_bar(d_gh, w_hh.t().contiguous(), dt, addend=d_h), what + " d_h")
    T.check(ts[2].grad, T.wgrad64(a, d_gi, dt), T.wgrad64(a, d_gi), T.wgrad_bar(a, d_gi, dt), what + " d_W_ih")
    T.check(ts[3].grad, T.wgrad64(h, d_gh, dt), T.wgrad64(h, d_gh), T.wgrad_bar(h, d_gh, dt), what + " d_W_hh")
    for got, d in ((ts[4].grad, d_gi), (ts[5].grad, d_gh)):               # bias gradients: the fp32 d_gi, d_gh, unrounded
        want = d.double().sum(dim=0)
        assert C.err(got, want) <= T.grad_bar(want), what


def test_gru_node_at_width_30_runs_the_fp32_kernels_alone():
    from ptgnn_amd import dense
    case = C.gru_case(60, 30, 30, 7503)      # widths off the fused cell's float4 rows: the two Linears + torch gate math
    ts = _cuda(*case)
    ref = [t.detach().clone().requires_grad_(True) for t in ts]
    for t in ts:
        t.requires_grad_(True)
    go = torch.randn(60, 30, generator=torch.Generator().manual_seed(7504)).cuda()
    out, since_f = _launches(lambda: dense.gru_cell_weights(*ts, inputs=torch.float16))
    _, since_b = _launches(lambda: out.backward(go))
    assert since_f and since_b and not [f for f in HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
    out0 = dense.gru_cell_weights(*ref)
    out0.backward(go)
    assert torch.equal(out, out0) and all(torch.equal(p.grad, q.grad) for p, q in zip(ts, ref))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the GGNN layer's training routes
# ---------------------------------------------------------------------------------------------------------------------
def _layer_case(dropout=0.0):
    """Table form: 200 nodes, 3 edge types, H = M = 64."""
    from ptgnn_amd import layers as L
    torch.manual_seed(8600)
    layer = L.GatedMessagePassingLayer(64, 64, 3, "sum", dropout_rate=dropout)
    x = torch.randn(200, 64, generator=torch.Generator().manual_seed(8601))
    adj = C.random_adjacency(200, (300, 200, 100), 8602)
    assert not L._prefer_edge_path(600, 200, 3, 64, 64)
    return layer.cuda(), x.cuda(), [(s.cuda(), d.cuda()) for s, d in adj]


def _step(layer, x, adj):
    """(output, gradients of every parameter and of the states, launches of the forward, launches of the backward)."""
    from ptgnn_amd import ops
    ops.clear_plan_cache()
    layer.zero_grad()
    x = x.detach().clone().requires_grad_(True)
    feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    out, since_f = _launches(lambda: layer(x, adj, None, {}, {}, feats))
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(8603)).to(out.device, out.dtype)
    _, since_b = _launches(lambda: out.backward(go))
    return out.detach(), [p.grad.clone() for p in layer.parameters()] + [x.grad.clone()], since_f, since_b


@DTYPES
def test_training_layer_takes_the_half_nodes_under_training_true(dt):
    import ptgnn_amd
    layer, x, adj = _layer_case()
    layer.train()
    default, default_grads, since_f, since_b = _step(layer, x, adj)
    assert not [f for f in HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
    # without the keyword: the default training bits, forward and gradients
    with ptgnn_amd.matrix_inputs(dt):
        got, grads, since_f, since_b = _step(layer, x, adj)
    assert not [f for f in HALF_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
    assert torch.equal(got, default) and all(torch.equal(p, q) for p, q in zip(grads, default_grads))
    with ptgnn_amd.matrix_inputs(torch.float32, training=True):                 # accepted, means fp32
        got, grads, since_f, since_b = _step(layer, x, adj)
    assert torch.equal(got, default) and all(torch.equal(p, q) for p, q in zip(grads, default_grads))
    # with it: the 16-bit nodes, forward and backward, and no fp32 GEMM family
    with ptgnn_amd.matrix_inputs(dt, training=True):
        got, grads, since_f, since_b = _step(layer, x, adj)
        again, again_grads, _, _ = _step(layer, x, adj)
        layer.eval()
        with torch.no_grad():
            feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
            inference = layer(x, adj, None, {}, {}, feats)
        layer.train()
    assert ptgnn_amd.get_matrix_inputs() is torch.float32
    assert since_f.get("half_linear") == 1 and since_f.get("half_gru_train") == 1, since_f
    assert since_b.get("half_linear") == 2 and since_b.get("half_linear_add") == 1 and since_b.get("half_wgrad") == 3, since_b
    assert not [f for f in T.FP32_GEMM_FAMILIES if f in since_f or f in since_b], (since_f, since_b)
    assert torch.equal(got, inference)                                          # the inference route's bits
    assert not torch.equal(got, default)
    assert torch.equal(again, got) and all(torch.equal(p, q) for p, q in zip(again_grads, grads))   # two calls, same bits
    # A sanity bound on the whole step (the stage tests above hold each GEMM to its bar): a gradient passes through at
    # most three rounded GEMMs, each moving its result by at most 2 u relative to the result's scale (u = 2^-9 for bf16,
    # 2^-12 for fp16, both operands rounded), and through the gate math's derivatives, which are at most 1: 6 u, with a
    # factor 4 of headroom for the scales of intermediate results against the final one.
    u = 2.0 ** -9 if dt is torch.bfloat16 else 2.0 ** -12
    for p, q in zip(grads, default_grads):
        assert not torch.equal(p, q)
        moved = float((p - q).abs().max())
        print(f"  gradient {tuple(q.shape)}: moved {moved:.3e}, scale {float(q.abs().max()):.3e}")
        assert moved <= 24 * u * max(1.0, float(q.abs().max()))


def test_per_edge_dropout_keeps_the_edge_gemm_fp32_and_rounds_the_gru_node():
    import ptgnn_amd
    layer, x, adj = _layer_case(dropout=0.2)
    layer.train()
    with ptgnn_amd.matrix_inputs(torch.bfloat16, training=True):
        _, _, since_f, since_b = _step(layer, x, adj)
    assert since_f.get("half_gru_train") == 1 and "half_linear" not in since_f, since_f
    assert [f for f in since_f if "edge" in f], since_f                                   # _EdgeLinear: an fp32 family
    assert since_b.get("half_wgrad") == 2 and since_b.get("half_linear_add") == 1 and since_b.get("half_linear") == 1, since_b
    assert [f for f in ("k_edge_wgrad", "k_wgrad_stream") if f in since_b], since_b       # _EdgeLinear's weight gradient
    assert [f for f in since_b if "edge" in f and "wgrad" not in f], since_b             # ... and its input gradient


def test_bf16_states_under_autocast_take_the_half_nodes_in_training():
    import ptgnn_amd
    layer, x, adj = _layer_case()
    layer.train()
    x_lo = x.to(torch.bfloat16)
    ptgnn_amd.set_matrix_inputs("autocast", training=True)
    try:
        _, _, outside_f, outside_b = _step(layer, x_lo, adj)                    # no autocast region: fp32
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got, grads, since_f, since_b = _step(layer, x_lo, adj)
        ptgnn_amd.set_matrix_inputs("autocast")                                 # without the keyword: fp32 in training
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, _, off_f, off_b = _step(layer, x_lo, adj)
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    assert not [f for f in HALF_FAMILIES if f in outside_f or f in outside_b], (outside_f, outside_b)
    assert not [f for f in HALF_FAMILIES if f in off_f or f in off_b], (off_f, off_b)
    assert since_f.get("half_linear") == 1 and since_f.get("half_gru_train") == 1, since_f
    assert since_b.get("half_wgrad") == 3 and since_b.get("half_linear_add") == 1, since_b
    assert got.dtype == torch.bfloat16 and grads[-1].dtype == torch.bfloat16
