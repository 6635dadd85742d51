"""The opt-in 16-bit GGNN message rows on the MI355X: csrc/gather_reduce16.hip behind `ops.gather_reduce`, the
row-storing producers behind `rows=` (ops.linear / ops.edge_linear / ops.edge_linear_shared), and the GGNN layer's
inference route under `ptgnn_amd.half_messages()`.

Bars.  Aggregation: max / min equal the float64 reduce of the same 16-bit rows bit for bit; sum / mean carry the bars of
tests/test_gpu_aggregation_paths.py for the same degrees -- rows of up to HUB_THRESHOLD in-edges the bits of the serial
fp32 fold in message order (oracle.scatter_ref), rows beyond it |got - float64| <= 5e-6 (1 + mass).  Producers: the bits
of the fp32-output launch's `.to(dtype)`.  Layer: the `bar` / `MARGIN` scheme of tests/half_cases.py, each stage against
float64 on the values that stage rounds (the messages the route stored, the aggregate it formed)."""
import pytest
import torch

import agg_paths as AP
import half_cases as C
from test_gpu_edge_inputs import (FP32_EDGE_FAMILIES, _check, _cuda_adj, _layer_case, _repeated_sources, _run,  # noqa: F401
                                  forms, unique_rows)

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
I32 = torch.int32
ROWS = (0, 1, 31, 32, 33, 97)                 # no row, one, both sides of a 32-row unit, a ragged fourth unit
# destination row -> in-degree: the groups of 8 and their clamped tails, kLongRow and one past it, one hub row; in and
# around the row range (32, 96) of the range test; every other row has 0 .. 6 in-edges
DEGREES = {3: 0, 33: 1, 40: 7, 41: 8, 95: 9, 96: 17, 50: AP.K_LONG_ROW, 100: AP.K_LONG_ROW + 1, 60: AP.HUB_THRESHOLD + 1}
N, T = 128, 3


def _since(fn):
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, half=True, edge16=True, rows16=True)
    out = fn()
    return out, ops.launches_since(before)


@pytest.fixture(scope="module")
def graph():
    """(plan, dst, src, typ in message order) of a T = 3 graph with the DEGREES above."""
    from ptgnn_amd import ops
    g = torch.Generator().manual_seed(4100)
    deg = torch.randint(0, 7, (N,), generator=g)
    for r, d in DEGREES.items():
        deg[r] = d
    dst = torch.repeat_interleave(torch.arange(N), deg)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, N, (dst.numel(),), generator=g)
    typ = torch.randint(0, T, (dst.numel(),), generator=g)
    adj = [(src[typ == t], dst[typ == t]) for t in range(T)]
    plan = ops.build_plan(_cuda_adj(adj), N)
    assert ops.HUB_THRESHOLD == AP.HUB_THRESHOLD and int(plan.hub_count.reshape(-1)[0]) > 0
    return plan, torch.cat([d for _, d in adj]), torch.cat([s for s, _ in adj]), \
        torch.cat([torch.full((int(s.shape[0]),), t) for t, (s, _) in enumerate(adj)]), deg


@DTYPES
@pytest.mark.parametrize("form", ["table", "rows"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("M", [32, 96, 256])
def test_aggregation_over_16_bit_rows_against_float64(graph, M, reduce, form, dt):
    from oracle import scatter_ref
    from ptgnn_amd import ops
    plan, dst, src, typ, deg = graph
    g = torch.Generator().manual_seed(M + 7)
    if form == "table":                         # [N, T M], column block t M of row src; the plan's own col / type_bits
        y16 = torch.randn(N, T * M, generator=g).to(dt)
        msgs16, kw = y16.view(N, T, M)[src, typ], {}
    else:                                       # one row per message, reached through `col`
        y16 = msgs16 = torch.randn(dst.numel(), M, generator=g).to(dt)
        kw = {"type_bits": 0, "col": plan.perm}
    yg = y16.cuda()
    out, since = _since(lambda: ops.gather_reduce(yg, plan, M, reduce, **kw))
    assert since == {"agg16": 1}, since
    part = torch.full((N, M), 7.0, device="cuda")
    assert ops.gather_reduce(yg, plan, M, reduce, out=part, rows=(32, 96), **kw) is part
    out, part = out.cpu(), part.cpu()
    assert torch.equal(part[32:96].view(I32), out[32:96].view(I32))
    assert bool((part[:32] == 7.0).all()) and bool((part[96:] == 7.0).all())
    want64 = AP.segment_ref(msgs16.double(), dst, N, reduce)
    if reduce in ("max", "min"):
        assert torch.equal(out.view(I32), want64.float().view(I32))
        return
    small = deg <= AP.HUB_THRESHOLD
    want32 = scatter_ref.scatter(msgs16.float(), dst, dim=0, dim_size=N, reduce=reduce)
    bad = (out.view(I32) != want32.view(I32)).any(1) & small
    assert not bool(bad.any()), ("serial-order bits", deg[bad].tolist())
    mass = scatter_ref.scatter(msgs16.double().abs(), dst, dim=0, dim_size=N, reduce=reduce)
    err = float((((out.double() - want64).abs() / (1.0 + mass))[~small]).max())
    print(f"  hub row {reduce} M={M} {form} {C.IDS[dt]}: |got - float64| / (1 + mass) = {err:.3e}")
    assert err <= 5e-6


@DTYPES
@pytest.mark.parametrize("h,m", [(h, m) for h in (32, 128, 256) for m in (32, 128, 256)])
def test_edge_producers_store_the_rounded_accumulators(unique_rows, dt, h, m):
    """Both launch forms (and, over the widths, both kernels behind them): rows16 == fp32-output launch .to(dt), and the
    shared rows equal the per-edge launch over the same (type, source) pairs."""
    from ptgnn_amd import ops
    n = 130
    cadj = _cuda_adj(_repeated_sources(n, ROWS, 3, 7300 + h + m))
    plan, uq = unique_rows(cadj, n)
    g = torch.Generator().manual_seed(h * m)
    x = torch.randn(n, h, generator=g).cuda()
    ws = [C.xavier(m, h, g).cuda() for _ in ROWS]
    live = sum(ROWS)
    shared, since = _since(lambda: ops.edge_linear_shared(x, uq, ws, inputs=dt, rows=dt))
    assert since == {"edge16_shared_rows16": 1} and shared.dtype == dt, since
    assert torch.equal(shared[:live], ops.edge_linear_shared(x, uq, ws, inputs=dt)[:live].to(dt))
    per_edge, since = _since(lambda: ops.edge_linear(x, cadj, ws, False, inputs=dt, rows=dt))
    assert since == {"edge16_rows16": 1} and per_edge.dtype == dt, since
    assert torch.equal(per_edge, ops.edge_linear(x, cadj, ws, False, inputs=dt).to(dt))
    assert torch.equal(ops.edge_linear(x, uq.adjacency(), ws, False, inputs=dt, rows=dt), shared[:live])


@DTYPES
@pytest.mark.parametrize("k,n_out", [(k, n) for k in (32, 128, 256) for n in (32, 128, 256)])
def test_linear_stores_the_rounded_accumulators(dt, k, n_out):
    from ptgnn_amd import ops
    g = torch.Generator().manual_seed(k + n_out)
    w, b = C.xavier(n_out, k, g).cuda(), torch.randn(n_out, generator=g).cuda()
    for rows in ROWS:
        x = torch.randn(rows, k, generator=g).cuda()
        y16, since = _since(lambda: ops.linear(x, w, b, inputs=dt, rows=dt))
        assert since == ({"linear_rows16": 1} if rows else {}) and y16.dtype == dt, since
        assert torch.equal(y16, ops.linear(x, w, b, inputs=dt).to(dt)), rows


@pytest.mark.parametrize("form", ["shared", "per_edge", "table"])
def test_layer_rounds_its_messages_once_under_the_switch(monkeypatch, forms, form):
    """bf16: message rounding moves this case's output by 157 bars; with fp16 by 13.7, short of the precondition's 20
    (computed from the two float64 references alone) -- fp16 rows are held bitwise at the producers and the aggregation
    above.  Switch off: the parent's launches and bits."""
    import ptgnn_amd
    from ptgnn_amd import layers as L, ops
    dt = torch.bfloat16
    layer, x, adj = _layer_case()
    weights = layer.export_weights()
    operands_only, _ = C.ggnn64(x, adj, weights, linear_dt=dt, gru_dt=dt)
    layer, xg, adjg = layer.cuda(), x.cuda(), _cuda_adj(adj)
    forms("shared" if form == "shared" else "per_edge")
    monkeypatch.setattr(L, "_prefer_edge_path", lambda *a: form != "table")
    producer = {"shared": "edge16_shared_rows16", "per_edge": "edge16_rows16", "table": "linear_rows16"}[form]
    with torch.no_grad(), ptgnn_amd.matrix_inputs(dt, edge_gemm=True):
        with C.captured(monkeypatch, ops, "gather_reduce") as parent_agg:
            parent, since = _since(lambda: _run(layer, xg, adjg))
        assert since.get("k_gather_reduce") == 1 and "agg16" not in since and producer not in since, since
        with ptgnn_amd.half_messages(), C.captured(monkeypatch, ops, "gather_reduce") as seen:
            got, since = _since(lambda: _run(layer, xg, adjg))
        assert since.get(producer) == 1 and since.get("agg16") == 1 and "k_gather_reduce" not in since, since
        assert not [f for f in FP32_EDGE_FAMILIES + ("edge16", "edge16_shared", "half_linear") if f in since], since
        with ptgnn_amd.half_messages(False), C.captured(monkeypatch, ops, "gather_reduce") as off_agg:
            off = _run(layer, xg, adjg)
        assert torch.equal(off, parent) and torch.equal(off_agg[0], parent_agg[0]) and not torch.equal(got, parent)
        ws = [w.cuda() for w in weights["edge_w"]]
        m16 = ops.edge_linear(xg, adjg, ws, False, inputs=dt, rows=dt)       # the rows either producer stores
    m64 = torch.cat([C.linear64(x, w, dt=dt)[s] for (s, _), w in zip(adj, weights["edge_w"])])
    e_msg = C.err(m16, m64)                                                   # one rounding of the fp32 accumulator
    assert e_msg <= C.bar(m64) + float(m64.abs().max()) * torch.finfo(dt).eps / 2, e_msg
    agg64 = C.aggregate64(m16.double().cpu(), torch.cat([d for _, d in adj]), x.shape[0], "sum")
    assert C.err(seen[0], agg64) <= C.bar(agg64)
    want = C.gru64(seen[0], x, weights["w_ih"], weights["w_hh"], weights["b_ih"], weights["b_hh"], dt=dt)
    _check(got, want, operands_only, f"layer {form} with bf16 message rows")


def test_an_unsupported_width_keeps_fp32_rows_and_ops_refuses_it(forms):
    import ptgnn_amd
    from ptgnn_amd import PtgnnAmdError, layers as L, ops
    n, counts = 300, (25,) * 8
    torch.manual_seed(1)
    layer = L.GatedMessagePassingLayer(64, 40, len(counts), "sum").eval().cuda()
    x, adj = torch.randn(n, 64).cuda(), _cuda_adj(C.random_adjacency(n, counts, 2))
    forms("per_edge")
    with torch.no_grad(), ptgnn_amd.matrix_inputs(torch.bfloat16, edge_gemm=True):
        want = _run(layer, x, adj)
        with ptgnn_amd.half_messages():
            got, since = _since(lambda: _run(layer, x, adj))
    assert torch.equal(got, want) and since.get("k_gather_reduce") == 1 and "agg16" not in since, since
    plan = ops.plan_for(adj, n)
    with pytest.raises(PtgnnAmdError, match="16-bit message rows"):
        ops.gather_reduce(torch.zeros(200, 40, dtype=torch.bfloat16, device="cuda"), plan, 40, "sum", type_bits=0,
                          col=plan.perm)
    with pytest.raises(PtgnnAmdError, match="16-bit message rows"):
        ops.gather_reduce(torch.zeros(200, 64, dtype=torch.bfloat16, device="cuda"), plan, 64, "max", type_bits=0,
                          col=plan.perm, return_arg=True)
