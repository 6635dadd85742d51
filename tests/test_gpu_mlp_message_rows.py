"""The opt-in 16-bit MLP-MP message rows on the MI355X: csrc/gather_reduce16_epi.hip behind `ops.gather_reduce` (a 16-bit
`ydst` and / or an epilogue), the per-edge GEMM with a target-state half storing 16-bit rows
(`ops.edge_linear(..., True, inputs=dt, rows=dt)`), and `MlpMessagePassingLayer`'s inference routes under
`ptgnn_amd.half_messages(mlp=True)`.

Bars.  Aggregation without an epilogue: max / min equal the fp32 fold of fp32(a) + fp32(b) bit for bit; sum / mean on
rows of up to HUB_THRESHOLD in-edges the serial fp32 fold of those sums in message order (oracle.scatter_ref), hub rows
|got - float64| <= 5e-6 (1 + mass) -- the bars of tests/test_gpu_message_rows.py.  With an epilogue: the attributed bar
of tests/test_gpu_aggregation_paths.py's fp32 epilogue test (agg_paths.attributed_ok against the fp32 and the float64
LayerNorm(GELU(.)) of the serial fp32 / float64 aggregate of the same up-cast values).  Producer: the bits of the
fp32-output launch's `.to(dtype)`.  Layer: the `bar` / `MARGIN` scheme of tests/half_cases.py, each stage against float64
on the values that stage rounds (the rows the producer stored, the aggregate the aggregation formed)."""
import pytest
import torch
import torch.nn.functional as F

import agg_paths as AP
import half_cases as C
import mlp_half_cases as MC
from test_gpu_message_rows import N, ROWS, T, _cuda_adj, _since, graph  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
I32 = torch.int32
# (form, M, epilogue): without a destination term and without an epilogue the call is the plain kernel's
CASES = [(f, m, e) for f in ("table_dst", "table", "rows") for m in (32, 96, 256) for e in ("none", "gelu_ln")
         if f == "table_dst" or e != "none"] + [(f, 96, "ln") for f in ("table_dst", "table", "rows")]


@DTYPES
@pytest.mark.parametrize("form,M,epi", CASES)
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_aggregation_with_destination_term_and_epilogue_against_float64(graph, reduce, form, M, epi, dt):
    from oracle import scatter_ref
    from ptgnn_amd import ops
    plan, dst, src, typ, deg = graph
    g = torch.Generator().manual_seed(M + 11)
    kw, b16 = {}, None
    if form == "rows":                          # one row per message, reached through `col`
        y16 = a16 = torch.randn(dst.numel(), M, generator=g).to(dt)
        kw = {"type_bits": 0, "col": plan.perm}
    else:                                       # [N, T M], column block t M of row src (+ block t M of row dst)
        y16 = torch.randn(N, T * M, generator=g).to(dt)
        a16 = y16.view(N, T, M)[src, typ]
        if form == "table_dst":
            yd16 = torch.randn(N, T * M, generator=g).to(dt)
            b16, kw = yd16.view(N, T, M)[dst, typ], {"ydst": yd16.cuda()}
    w, b = torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g)
    flags = {"none": ops.EPI_NONE, "ln": ops.EPI_LAYERNORM, "gelu_ln": ops.EPI_GELU_LAYERNORM}[epi]
    if flags:
        kw.update(epilogue=flags, ln_weight=w.cuda(), ln_bias=b.cuda())
    yg = y16.cuda()
    out, since = _since(lambda: ops.gather_reduce(yg, plan, M, reduce, **kw))
    assert since == {"agg16_epi": 1}, since
    part = torch.full((N, M), 7.0, device="cuda")
    assert ops.gather_reduce(yg, plan, M, reduce, out=part, rows=(32, 96), **kw) is part
    out, part = out.cpu(), part.cpu()
    assert torch.equal(part[32:96].view(I32), out[32:96].view(I32))
    assert bool((part[:32] == 7.0).all()) and bool((part[96:] == 7.0).all())

    m32 = a16.float() if b16 is None else a16.float() + b16.float()           # one IEEE addition per slot
    m64 = a16.double() if b16 is None else a16.double() + b16.double()
    if reduce in ("max", "min"):
        a32 = AP.segment_ref(m32, dst, N, reduce)
        a64 = AP.segment_ref(m64, dst, N, reduce)
    else:
        a32 = scatter_ref.scatter(m32, dst, dim=0, dim_size=N, reduce=reduce)
        a64 = scatter_ref.scatter(m64, dst, dim=0, dim_size=N, reduce=reduce)
    if flags:
        def finish(a):
            a = F.gelu(a) if flags & ops.EPI_GELU else a
            return F.layer_norm(a, (M,), w.to(a.dtype), b.to(a.dtype), eps=1e-5)
        assert AP.attributed_ok(out, finish(a32), finish(a64)), (reduce, form, M, epi)
        return
    if reduce in ("max", "min"):
        assert torch.equal(out.view(I32), a32.view(I32))
        return
    small = deg <= AP.HUB_THRESHOLD
    bad = (out.view(I32) != a32.view(I32)).any(1) & small
    assert not bool(bad.any()), ("serial-order bits", deg[bad].tolist())
    mass = scatter_ref.scatter(m64.abs(), dst, dim=0, dim_size=N, reduce=reduce)
    err = float((((out.double() - a64).abs() / (1.0 + mass))[~small]).max())
    print(f"  hub row {reduce} M={M} {form} {C.IDS[dt]}: |got - float64| / (1 + mass) = {err:.3e}")
    assert err <= 5e-6


def test_aggregation_refuses_what_it_does_not_take(graph):
    from ptgnn_amd import PtgnnAmdError, ops
    plan = graph[0]
    y16 = torch.zeros(N, T * 64, dtype=torch.bfloat16, device="cuda")
    for bad in (dict(ydst=y16.float()), dict(ydst=y16.to(torch.float16)), dict(ydst=y16, return_arg=True)):
        with pytest.raises(PtgnnAmdError, match="16-bit message rows"):
            ops.gather_reduce(y16, plan, 64, "max", **bad)
    with pytest.raises(PtgnnAmdError, match="16-bit message rows"):
        ops.gather_reduce(y16.float(), plan, 64, "sum", ydst=y16)
    wide = torch.zeros(N, T * 288, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(PtgnnAmdError, match="16-bit message rows"):
        ops.gather_reduce(wide, plan, 288, "sum", ydst=wide)


@DTYPES
@pytest.mark.parametrize("h,m", [(h, m) for h in (32, 128, 256) for m in (32, 128, 256)])
def test_producer_with_a_target_half_stores_the_rounded_accumulators(dt, h, m):
    from ptgnn_amd import ops
    n = 130
    cadj = _cuda_adj(MC.adjacency(n, ROWS, 7400 + h + m))
    g = torch.Generator().manual_seed(h * m + 1)
    x = torch.randn(n, h, generator=g).cuda()
    ws = [C.xavier(m, 2 * h, g).cuda() for _ in ROWS]
    rows16, since = _since(lambda: ops.edge_linear(x, cadj, ws, True, inputs=dt, rows=dt))
    assert since == {"edge16_dst_rows16": 1} and rows16.dtype == dt and rows16.shape == (sum(ROWS), m), since
    assert torch.equal(rows16, ops.edge_linear(x, cadj, ws, True, inputs=dt).to(dt))


def _layer_launches(fn):
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, half=True, edge16=True, edge16_dst=True, rows16=True)
    out = fn()
    return out, ops.launches_since(before)


LAYER_KEYS = [k for k in MC.LAYER_SEEDS if k[1] == 128]


@DTYPES
@pytest.mark.parametrize("key", LAYER_KEYS, ids=lambda k: f"{k[0]}-{k[2]}-{'dst' if k[3] else 'src'}")
def test_layer_stores_and_aggregates_16_bit_rows_under_the_switch(monkeypatch, dt, key):
    """The launches are the row-storing producer and the new aggregation (this fails without the feature); each stage is
    inside the bar of float64 on the values it rounds; every other setting keeps the parent route's bits."""
    import ptgnn_amd
    from ptgnn_amd import ops
    form, hidden, reduce, use_dst = key
    layer, x, adj = MC.layer_case(form, hidden, reduce, use_dst, MC.LAYER_SEEDS[key])
    weights = layer.export_weights()
    ws = [w[0] for w in weights["edge_mlp"]]
    layer, xg, adjg = layer.cuda(), x.cuda(), _cuda_adj(adj)
    n = x.shape[0]
    producer_fn = "linear" if form == "table" else "edge_linear"
    producer = "linear_rows16" if form == "table" else ("edge16_dst_rows16" if use_dst else "edge16_rows16")
    with torch.no_grad():
        default = MC.run_layer(layer, xg, adjg)
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            parent, since = _layer_launches(lambda: MC.run_layer(layer, xg, adjg))
            assert since.get("k_gather_reduce") == 1 and not [f for f in since if "rows16" in f or "agg16" in f], since
            with ptgnn_amd.half_messages():                       # the GGNN switch alone: the parent's bits
                assert torch.equal(MC.run_layer(layer, xg, adjg), parent)
            with ptgnn_amd.half_messages(mlp=True), C.captured(monkeypatch, ops, producer_fn) as stored, \
                    C.captured(monkeypatch, ops, "gather_reduce") as seen:
                got, since = _layer_launches(lambda: MC.run_layer(layer, xg, adjg))
        assert since.get(producer) == 1 and since.get("agg16_epi") == 1, since
        assert not [f for f in ("k_gather_reduce", "k_gather_update", "agg16", "half_linear", "edge16", "edge16_dst")
                    if f in since], since
        with ptgnn_amd.half_messages(mlp=True):                   # without `mlp=True` on the matrix inputs: fp32
            with ptgnn_amd.matrix_inputs(dt):
                assert torch.equal(MC.run_layer(layer, xg, adjg), default)
        assert not torch.equal(got, parent)
    with ptgnn_amd.matrix_inputs(dt, mlp=True), ptgnn_amd.half_messages(mlp=True):      # a gradient is needed: fp32
        assert torch.equal(MC.run_layer(layer, xg, adjg).detach(), default)

    # stage 1: the stored rows are one rounding of the 16-bit GEMM's accumulator
    rows16 = stored[0].cpu()
    targets, types = torch.cat([d for _, d in adj]), torch.cat([torch.full((int(s.numel()),), t) for t, (s, _) in
                                                                enumerate(adj)])
    if form == "table":
        xr = C.rnd64(x, dt)
        halves = [w[:, :hidden] for w in ws] + ([w[:, hidden:] for w in ws] if use_dst else [])
        m64 = xr @ C.rnd64(torch.cat(halves), dt).t()
        src = torch.cat([s for s, _ in adj])
        up = rows16.double().view(n, -1, hidden)
        msgs = up[src, types] + (up[targets, len(adj) + types] if use_dst else 0.0)
    else:
        m64 = MC.messages64(x, adj, ws, use_dst, dt)
        msgs = rows16.double()
    assert rows16.dtype == dt and C.err(rows16, m64) <= C.bar(m64) + float(m64.abs().max()) * torch.finfo(dt).eps / 2
    # stage 2: aggregate + GELU + LayerNorm of exactly those rows
    agg64 = F.layer_norm(F.gelu(C.aggregate64(msgs, targets, n, reduce)), (hidden,), weights["ln_w"].double(),
                         weights["ln_b"].double(), 1e-5)
    assert seen[0].dtype == torch.float32 and C.err(seen[0], agg64) <= C.bar(agg64)
    # stage 3: the fp32 dense update of that aggregate; the route is MARGIN bars from the one that rounds operands only
    want = torch.tanh(seen[0].double().cpu() @ weights["dense_w"].double().t() + weights["dense_b"].double())
    operands_only = MC.mlp64(x, adj, weights, dt=dt)
    MC.check(got, want, operands_only, f"layer {key} with {C.IDS[dt]} message rows")
    assert C.err(parent, operands_only) <= C.bar(operands_only)


@DTYPES
def test_one_launch_update_route_at_hidden_64_keeps_its_fp32_rows(dt):
    import ptgnn_amd
    key = ("edge", 64, "sum", True)
    layer, x, adj = MC.layer_case(*key, MC.LAYER_SEEDS[key])
    layer, xg, adjg = layer.cuda(), x.cuda(), _cuda_adj(adj)
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt, mlp=True):
        parent = MC.run_layer(layer, xg, adjg)
        with ptgnn_amd.half_messages(mlp=True):
            got, since = _layer_launches(lambda: MC.run_layer(layer, xg, adjg))
    assert torch.equal(got, parent) and since.get("k_gather_update") == 1 and since.get("edge16_dst") == 1, since
    assert not [f for f in since if "rows16" in f or "agg16" in f], since
