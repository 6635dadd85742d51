"""The opt-in 16-bit message and gradient rows of the GGNN edge-form training step on the MI355X
(`half_messages(training=True)` on top of `matrix_inputs(dt, edge_training=True)`): csrc/segment_reduce16.hip behind
`ops.segment_reduce16` / `ops.segment_spread16`, the 16-bit-source and 16-bit-store forms of csrc/edge_gemm16.hip and
csrc/edge_wgrad16.hip behind `ops.edge_linear` / `ops.edge_weight_grad`, and the layer route.

Bars.  Aggregation: those of tests/test_gpu_message_rows.py (max / min the bits of the float64 reduce; sums of rows up to
HUB_THRESHOLD the bits of the serial fp32 fold, beyond it 5e-6 (1 + mass)); the arg equals the fp32 kernel's on the up-cast
rows.  Spread, 16-bit sources and 16-bit stores: bit equality with the fp32-row launch (its `.to(dtype)` for the stores).
Gradient GEMMs and the layer: C.bar / T.floored_bar against float64 on the values each stage rounds."""
import ctypes

import pytest
import torch

import agg_paths as AP
import edge_training_cases as E
import half_cases as C
import half_training_cases as T

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
I32 = torch.int32
SEED = E.SEED
N, TYPES = 128, 3
# destination row -> in-degree (the table of tests/test_gpu_message_rows.py): the groups of 8 and their clamped tails,
# kLongRow and one past it, one hub row; every other row has 0 .. 6 in-edges
DEGREES = {3: 0, 33: 1, 40: 7, 41: 8, 95: 9, 96: 17, 50: AP.K_LONG_ROW, 100: AP.K_LONG_ROW + 1, 60: AP.HUB_THRESHOLD + 1}
TIED = (41, 100, 60)          # one row per path (lane group, beyond kLongRow, hub) whose messages are all equal


def _cuda_adj(adj):
    return [(s.cuda(), d.cuda()) for s, d in adj]


def _since(fn):
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, edge16=True, edge16_training=True, rows16=True)
    out = fn()
    return out, ops.launches_since(before)


@pytest.fixture(scope="module")
def graph():
    """(plan, dst in message order, in-degrees) of a T = 3 graph with the DEGREES above; E % 8 == 5."""
    from ptgnn_amd import ops
    g = torch.Generator().manual_seed(4100)
    deg = torch.randint(0, 7, (N,), generator=g)
    for r, d in DEGREES.items():
        deg[r] = d
    deg[0] += (5 - int(deg.sum())) % 8
    dst = torch.repeat_interleave(torch.arange(N), deg)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, N, (dst.numel(),), generator=g)
    typ = torch.randint(0, TYPES, (dst.numel(),), generator=g)
    adj = [(src[typ == t], dst[typ == t]) for t in range(TYPES)]
    plan = ops.build_plan(_cuda_adj(adj), N)
    assert ops.HUB_THRESHOLD == AP.HUB_THRESHOLD and plan.num_edges % 8 == 5
    return plan, torch.cat([d for _, d in adj]), deg


def _messages(dst, M, dt, seed):
    msgs = torch.randn(dst.numel(), M, generator=torch.Generator().manual_seed(seed))
    for r in TIED:
        msgs[dst == r] = 1.5
    return msgs.to(dt)


@DTYPES
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("M", [32, 96, 256])
def test_aggregation_with_arg_and_spread_over_16_bit_rows(graph, M, reduce, dt):
    from oracle import scatter_ref
    from ptgnn_amd import ops
    plan, dst, deg = graph
    msgs16 = _messages(dst, M, dt, M + 7)
    yg = msgs16.cuda()
    minmax = reduce in ("max", "min")
    res, since = _since(lambda: ops.segment_reduce16(yg, plan, reduce, return_arg=minmax))
    assert since == {"segment_reduce16": 1}, since
    out = (res[0] if minmax else res).cpu()
    want64 = AP.segment_ref(msgs16.double(), dst, N, reduce)
    rowptr, perm = plan.rowptr.cpu().long(), plan.perm.cpu().long()[:plan.num_edges]
    arg = None
    if minmax:
        assert torch.equal(out.view(I32), want64.float().view(I32))
        arg = res[1]
        assert torch.equal(arg, ops.gather_reduce(yg.float(), plan, M, reduce, return_arg=True, type_bits=0,
                                                  col=plan.perm)[1])
        a = arg.cpu().long()
        empty = (deg == 0).unsqueeze(1).expand_as(a)
        assert bool((a[empty] == -1).all()) and bool((a[~empty] >= 0).all())
        inside = (a >= rowptr[:-1, None]) & (a < rowptr[1:, None])
        held = msgs16.float()[perm[a.clamp(min=0)], torch.arange(M).expand_as(a)]
        assert bool(inside[~empty].all()) and torch.equal(held[~empty], out[~empty])
        for r in TIED:                                   # an exact tie: the earliest slot of the row
            assert bool((a[r] == rowptr[r]).all()), r
    else:
        small = deg <= AP.HUB_THRESHOLD
        want32 = scatter_ref.scatter(msgs16.float(), dst, dim=0, dim_size=N, reduce=reduce)
        bad = (out.view(I32) != want32.view(I32)).any(1) & small
        assert not bool(bad.any()), ("serial-order bits", deg[bad].tolist())
        mass = scatter_ref.scatter(msgs16.double().abs(), dst, dim=0, dim_size=N, reduce=reduce)
        err = float((((out.double() - want64).abs() / (1.0 + mass))[~small]).max())
        print(f"  hub row {reduce} M={M} {C.IDS[dt]}: |got - float64| / (1 + mass) = {err:.3e}")
        assert err <= 5e-6

    # the spread of a row gradient back onto the messages, as 16-bit rows.  mean: the kernel multiplies by the fp32
    # reciprocal 1.0f / deg (one IEEE division, one multiply per value), restated here on the CPU
    g = torch.randn(N, M, generator=torch.Generator().manual_seed(M + 11))
    gs = g * (1.0 / deg.clamp(min=1).float()).unsqueeze(1) if reduce == "mean" else g
    got, since = _since(lambda: ops.segment_spread16(g.cuda(), arg, plan, reduce, dt))
    assert since == {"segment_spread16": 1} and got.dtype == dt, since
    assert torch.equal(got, ops.segment_spread(gs.cuda(), arg, plan).to(dt))
    want = gs.double()[dst]
    if minmax:
        slot_of = torch.empty(plan.num_edges, dtype=torch.long)
        slot_of[perm] = torch.arange(plan.num_edges)
        want = torch.where(arg.cpu().long()[dst] == slot_of.unsqueeze(1), want, torch.zeros((), dtype=torch.float64))
    assert torch.equal(got.cpu(), want.to(dt))


def _identity(plan):
    return [(i, i) for i in plan.identity_index()]


@DTYPES
@pytest.mark.parametrize("p", [0.0, E.P])
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_gradient_gemms_read_16_bit_gradient_rows(dt, h, m, p):
    from ptgnn_amd import ops
    x, ws, adj, g = E.edge_case(h, m)
    g16 = g.to(dt)
    n_edges = g.shape[0]
    cadj = _cuda_adj(adj)
    ops.clear_plan_cache()
    plan = ops.plan_for(cadj, E.N)
    bits = ops.dropout_bitmask(n_edges, h, p, SEED, "cuda") if p else None
    keep = E.unpack(bits, h) if p else None
    refs = E.references(x, ws, adj, g16.float(), keep, p, dt)
    xg, gg = x.cuda(), g16.cuda()
    what = f"{C.IDS[dt]} ({h}, {m}) p={p}"

    d_w, since = _since(lambda: ops.edge_weight_grad(xg, cadj, gg, False, p, SEED, mask_bits=bits, inputs=dt))
    assert since == {"edge_wgrad16_rows16": 1}, since
    assert torch.equal(d_w, ops.edge_weight_grad(xg, cadj, gg.float(), False, p, SEED, mask_bits=bits, inputs=dt))
    e = C.err(d_w, refs["d_w"][0])
    print(f"  {what} d_w: {e:.3e} (bar {refs['d_w'][2]:.3e})")
    assert e <= refs["d_w"][2]

    wts = [w.t().contiguous().cuda() for w in ws]
    drop = (2, p, SEED) if p else None
    g_in, since = _since(lambda: ops.edge_linear(gg, _identity(plan), wts, False, dropout=drop, mask_bits=bits, inputs=dt))
    assert since == {"edge16_train_rows16": 1} and g_in.dtype == torch.float32, since
    assert torch.equal(g_in, ops.edge_linear(gg.float(), _identity(plan), wts, False, dropout=drop, mask_bits=bits,
                                             inputs=dt))
    e = C.err(g_in, refs["g_in"][0])
    print(f"  {what} g_in: {e:.3e} (bar {refs['g_in'][2]:.3e})")
    assert e <= refs["g_in"][2]
    # the 16-bit store of the same launch: rounded once, after mask and scale
    g_in16, since = _since(lambda: ops.edge_linear(gg, _identity(plan), wts, False, dropout=drop, mask_bits=bits,
                                                   inputs=dt, rows=dt))
    assert since == {"edge16_train_rows16": 1} and torch.equal(g_in16, g_in.to(dt)), since


def _entry(x, x16, adj, w16, dt, out, out16, mode, p, bits):
    """ptgnn_amd_edge_train_rows16_linear16 into a caller-owned (strided) `out`."""
    from ptgnn_amd import _lib, ops
    lib = _lib.load()
    t = len(adj)
    srcs = [s.contiguous() for s, _ in adj]
    sp = (ctypes.c_void_p * t)(*[s.data_ptr() if s.numel() else None for s in srcs])
    cn = (ctypes.c_int64 * t)(*[int(s.shape[0]) for s in srcs])
    rc = lib.ptgnn_amd_edge_train_rows16_linear16(
        x.data_ptr(), int(x16), x.stride(0), x.shape[0], x.shape[1], ctypes.cast(sp, ctypes.c_void_p),
        ctypes.cast(cn, ctypes.c_void_p), w16.data_ptr(), t, w16.shape[1], ops.HALF_IDS[dt], out.data_ptr(), int(out16),
        out.stride(0), mode, float(p), bits.data_ptr(), ops._stream(out))
    _lib.check(rc, "ptgnn_amd_edge_train_rows16_linear16")
    return out


@DTYPES
@pytest.mark.parametrize("h,m", E.EDGE_SHAPES)
def test_masked_gemm_stores_16_bit_rows_inside_a_strided_view(dt, h, m):
    """Mode 1 (the forward with dropout) and mode 2 (the input gradient): rows16 == fp32-output launch .to(dt), written
    into a column slice of a NaN-filled buffer that stays NaN everywhere else."""
    from ptgnn_amd import ops
    x, ws, adj, g = E.edge_case(h, m)
    n_edges = g.shape[0]
    cadj = _cuda_adj(adj)
    plan = ops.plan_for(cadj, E.N)
    xg, gg = x.cuda(), g.to(dt).cuda()
    wsg = [w.cuda() for w in ws]
    bits = ops.dropout_bitmask(n_edges, h, E.P, SEED, "cuda")
    fwd = ops.edge_linear(xg, cadj, wsg, False, dropout=(1, E.P, SEED), mask_bits=bits, inputs=dt)
    wts = [w.t().contiguous() for w in wsg]
    bwd = ops.edge_linear(gg, _identity(plan), wts, False, dropout=(2, E.P, SEED), mask_bits=bits, inputs=dt)
    cases = ((xg, False, cadj, torch.stack(wsg), 1, fwd), (gg, True, _identity(plan), torch.stack(wts), 2, bwd))
    for src, src16, ids, stack, mode, want in cases:
        buf = torch.full((n_edges, want.shape[1] + 16), float("nan"), device="cuda").to(dt)
        view = buf[:, 8:8 + want.shape[1]]
        _, since = _since(lambda: _entry(src, src16, ids, stack.to(dt).contiguous(), dt, view, True, mode, E.P, bits))
        assert since == {"edge16_train_rows16": 1}, since
        assert torch.equal(view, want.to(dt)), mode
        assert bool(buf[:, :8].isnan().all()) and bool(buf[:, 8 + want.shape[1]:].isnan().all()), mode
    got = ops.edge_linear(xg, cadj, wsg, False, dropout=(1, E.P, SEED), mask_bits=bits, inputs=dt, rows=dt)
    assert torch.equal(got, fwd.to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# the GGNN layer's edge-form training branch
# ---------------------------------------------------------------------------------------------------------------------
H, COUNTS, NODES = 64, (100, 90, 80, 70, 0, 60, 33, 1), 200       # an edge-form batch also without dropout


def _layer_case(dropout, agg):
    from ptgnn_amd import layers as L
    torch.manual_seed(9700)
    layer = L.GatedMessagePassingLayer(H, H, len(COUNTS), agg, dropout_rate=dropout).train()
    x = torch.randn(NODES, H, generator=torch.Generator().manual_seed(9701))
    return layer, x, C.random_adjacency(NODES, COUNTS, 9702)


def _step(layer, x, adj, go):
    from ptgnn_amd import ops
    ops.clear_plan_cache()
    layer.zero_grad()
    torch.manual_seed(9703)
    x = x.detach().clone().requires_grad_(True)
    feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    out, since_f = _since(lambda: layer(x, adj, None, {}, {}, feats))
    _, since_b = _since(lambda: out.backward(go))
    return out.detach(), [p.grad.clone() for p in layer.parameters()] + [x.grad.clone()], since_f, since_b


def _restated(weights, x, adj, keep, p, dt, agg, go, hp):
    """The step in precision `hp` (float64: the reference; float32: what the floored bars compare it with), rounding to
    `dt` at the route's four points: the GEMM operands, the messages, grad_msg and the per-edge input gradient.  Returns
    (output, d_x, d_w [T, M, H])."""
    counts = [int(s.shape[0]) for s, _ in adj]
    dst = torch.cat([d for _, d in adj])

    def rnd(t):
        return t.detach().to(dt).to(hp)

    rows = [rnd(r) for r in E.split(E.dropped(E.gathered(x, adj), keep, p), counts)]
    ws = [rnd(w) for w in weights["edge_w"]]
    msg = rnd(torch.cat([r @ w.t() for r, w in zip(rows, ws)])).requires_grad_(True)
    h = x.detach().to(hp).requires_grad_(True)
    a = AP.segment_ref(msg, dst, x.shape[0], agg)
    w_ih, w_hh, b_ih, b_hh = (weights[k].detach().to(hp) for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
    gi, gh = a @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    out = (1.0 - z) * torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]) + z * h
    out.backward(go.to(hp))
    gm = E.split(rnd(msg.grad), counts)
    d_w = torch.stack([g_t.t() @ r_t for g_t, r_t in zip(gm, rows)])
    g_in = torch.cat([g_t @ w for g_t, w in zip(gm, ws)])
    if keep is not None:
        g_in = g_in * keep.to(hp) * E.scale32(p)
    return out.detach(), h.grad + E.source_sum(rnd(g_in), adj, x.shape[0]), d_w


@DTYPES
@pytest.mark.parametrize("agg", ["max", "sum"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layer_keeps_its_edge_rows_16_bit_under_the_keyword(monkeypatch, dt, agg, p):
    import ptgnn_amd
    from ptgnn_amd import ops
    from ptgnn_amd import layers as L
    assert L._prefer_edge_path(sum(COUNTS), NODES, len(COUNTS), H, H)
    layer, x, adj = _layer_case(p, agg)
    weights = layer.export_weights()
    go = torch.randn(NODES, H, generator=torch.Generator().manual_seed(9704))
    layer, xg, adjg, gog = layer.cuda(), x.cuda(), _cuda_adj(adj), go.cuda()
    with ptgnn_amd.matrix_inputs(dt, edge_training=True):
        parent, parent_grads, par_f, par_b = _step(layer, xg, adjg, gog)
        with ptgnn_amd.half_messages():                   # no keyword: the parent's launches and bits
            plain, plain_grads, plain_f, plain_b = _step(layer, xg, adjg, gog)
        with ptgnn_amd.half_messages(training=True), C.captured(monkeypatch, ops, "segment_spread") as spreads:
            got, grads, since_f, since_b = _step(layer, xg, adjg, gog)
    assert torch.equal(plain, parent) and all(torch.equal(a, b) for a, b in zip(plain_grads, parent_grads))
    assert (plain_f, plain_b) == (par_f, par_b), (plain_f, par_f, plain_b, par_b)
    producer = "edge16_train_rows16" if p else "edge16_rows16"
    assert since_f.get(producer) == 1 and since_f.get("segment_reduce16") == 1, since_f
    assert since_b.get("segment_spread16") == 1 and since_b.get("edge_wgrad16_rows16") == 1, since_b
    assert since_b.get("edge16_train_rows16") == 1 and since_b.get("agg16") == 1, since_b
    stale = ("k_gather_reduce", "edge16_masked", "edge_wgrad16", "edge16") + E.FP32_EDGE_FAMILIES
    assert not spreads and not [f for f in stale if f in since_f or f in since_b], (since_f, since_b)

    keep = None
    if p:
        torch.manual_seed(9703)                          # the seed the layer drew (layers._dropout_seed)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        keep = E.unpack(ops.dropout_bitmask(sum(COUNTS), H, p, seed, "cuda"), H)
    want = _restated(weights, x, adj, keep, p, dt, agg, go, torch.float64)
    want32 = _restated(weights, x, adj, keep, p, dt, agg, go, torch.float32)
    d_w = grads[0:len(COUNTS)]
    for name, g, w64, w32 in (("output", got, want[0], want32[0]), ("d_x", grads[-1], want[1], want32[1]),
                              ("d_w", torch.stack(d_w), want[2], want32[2])):
        e, bar = C.err(g, w64), T.floored_bar(w64, w32)
        print(f"  {C.IDS[dt]} {agg} p={p} {name}: {e:.3e} (bar {bar:.3e})")
        assert e <= bar, name
