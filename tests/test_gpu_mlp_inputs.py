"""The opt-in 16-bit matrix inputs of the MLP-MP layer on the MI355X: the grouped per-edge GEMM with a target-state half
(csrc/edge_gemm16.hip: ptgnn_amd_edge_dst_linear16) through `ops.edge_linear(..., use_dst=True, inputs=)`, and
`MlpMessagePassingLayer`'s inference routes -- table form and edge form, string aggregations and PNA -- under
`ptgnn_amd.matrix_inputs(dtype, mlp=True)`.

Reference: float64 on the ROUNDED message operands; bar: TOL * max(1, |want|inf) (tests/half_cases.py says why that bar
holds for 16-bit operands; tests/mlp_half_cases.py how the layer cases were chosen).  Every numeric test first asserts,
from the two float64 references alone, that rounding moves the result by at least 20 bars, and then that the result is
within one bar of the rounded reference and at least `gap - bar` from the exact one.

Two kernels sit behind the entry (weight-stationary for H in {64, 128} with M <= 128 -- a chain of 2 H in {128, 256} --
per-wave otherwise); the shapes below put every test on both sides of that split and of the M <= 128 bound."""
import ctypes

import pytest
import torch

import half_cases as C
import mlp_half_cases as MC

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
HALF_FAMILIES = ("half_linear", "edge16", "edge16_shared", "edge16_dst")
FP32_EDGE_FAMILIES = ("k_stream_edge", "k_stream_edge_shared", "k_stream_edge_v2", "k_edge_linear")
FP32_LINEAR_FAMILIES = ("k_stream_linear", "k_stream_linear_ring", "k_linear_tlp")
EINVAL, EUNSUPPORTED = -1, -2


def _launches(fn):
    """(result of fn, {family: launches it made}) over the GEMM, the aggregation, the half and both edge16 ranges."""
    from ptgnn_amd import ops
    before = ops.launch_counts(aggregation=True, half=True, edge16=True, edge16_dst=True)
    out = fn()
    return out, ops.launches_since(before)


def _cuda_adj(adj):
    return [(s.cuda(), d.cuda()) for s, d in adj]


# ---------------------------------------------------------------------------------------------------------------------
# the entry: exact integer data -- the fragment maps, the two halves, the unit decode, row tails, empty types
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_messages_are_exact_on_integer_data(dt):
    """x in [-8, 8], W in [-2, 2]: every partial sum is an integer below 2^24, so the 16-bit launch must give the very
    bits of the fp32 launch and of the torch product.  src != dst on every edge and W^s != W^d: swapped halves, a target
    list read at the wrong offset or a wrong unit decode cannot pass."""
    from ptgnn_amd import ops
    n = MC.N_NODES
    adj = MC.adjacency(n, MC.UNIT_ROWS, 8100)
    cadj = _cuda_adj(adj)
    for h in (32, 64, 128, 256):
        for m in (32, 64, 160):
            g = torch.Generator().manual_seed(8200 + h + m)
            x = torch.randint(-8, 9, (n, h), generator=g).float()
            ws = [torch.randint(-2, 3, (m, 2 * h), generator=g).float() for _ in MC.UNIT_ROWS]
            xg, wg = x.cuda(), [w.cuda() for w in ws]
            got, since = _launches(lambda: ops.edge_linear(xg, cadj, wg, True, inputs=dt))
            assert since == {"edge16_dst": 1}, since
            want = ops.edge_linear(xg, cadj, wg, True)                                # the fp32 launch, same rows
            assert got.shape == want.shape and torch.equal(got, want), (C.IDS[dt], h, m)
            ref = torch.cat([torch.cat([x[s], x[d]], dim=1) @ w.t() for (s, d), w in zip(adj, ws)])
            assert torch.equal(got.cpu(), ref), (C.IDS[dt], h, m)


# ---------------------------------------------------------------------------------------------------------------------
# random data against float64 on the rounded operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    """(H, M) -> (x, weights, adjacency): N(0, 1) states, Xavier [M, 2 H] weights; built once, never changed."""
    out = {}
    for h in (64, 128, 256):
        for m in (64, 160):
            g = torch.Generator().manual_seed(8300 + h + m)
            x = torch.randn(MC.N_NODES, h, generator=g)
            ws = [C.xavier(m, 2 * h, g) for _ in MC.UNIT_ROWS]
            out[h, m] = (x, ws, MC.adjacency(MC.N_NODES, MC.UNIT_ROWS, 8310 + h + m))
    return out


@DTYPES
@pytest.mark.parametrize("h", [64, 128, 256])
@pytest.mark.parametrize("m", [64, 160])
def test_messages_match_float64_on_the_rounded_operands(random_cases, dt, h, m):
    from ptgnn_amd import ops
    x, ws, adj = random_cases[h, m]
    xg, wg, cadj = x.cuda(), [w.cuda() for w in ws], _cuda_adj(adj)
    got, since = _launches(lambda: ops.edge_linear(xg, cadj, wg, True, inputs=dt))
    assert since == {"edge16_dst": 1}, since
    MC.check(got, MC.messages64(x, adj, ws, dt=dt), MC.messages64(x, adj, ws), f"messages {C.IDS[dt]} H={h} M={m}")
    stack = torch.stack([w.to(dt) for w in wg])                                       # a rounded stack from the caller
    given, since = _launches(lambda: ops.edge_linear(xg, cadj, wg, True, inputs=dt, rounded=stack))
    assert since == {"edge16_dst": 1} and torch.equal(given, got)
    tanh = ops.edge_linear(xg, cadj, wg, True, act="tanh", inputs=dt)                 # the activation rides the store
    want = MC.messages64(x, adj, ws, dt=dt, act="tanh")
    assert C.err(tanh, want) <= C.bar(want)


# ---------------------------------------------------------------------------------------------------------------------
# row independence
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("h,m", [(64, 64), (128, 128), (64, 160), (96, 64), (256, 128)])
def test_rows_do_not_depend_on_the_launch_they_are_in(dt, h, m):
    """The same (src, dst, type) edges in two adjacencies with other counts and positions -- a launch over all edges, and
    two launches over a part each, whose 32-row units end elsewhere -- give the same bits per edge, in both kernels'
    shape classes; and two identical calls give the same bits."""
    from ptgnn_amd import ops
    n = MC.N_NODES
    g = torch.Generator().manual_seed(8500 + h + m)
    x = torch.randn(n, h, generator=g).cuda()
    ws = [C.xavier(m, 2 * h, g).cuda() for _ in range(4)]
    cadj = _cuda_adj(MC.adjacency(n, (210, 0, 99, 387), 8501))
    whole = ops.edge_linear(x, cadj, ws, True, inputs=dt)
    assert torch.equal(whole, ops.edge_linear(x, cadj, ws, True, inputs=dt))
    cut = [int(s.numel()) * 2 // 5 for s, _ in cadj]                  # 84, 0, 39, 154 rows: units end elsewhere
    first = ops.edge_linear(x, [(s[:c], d[:c]) for (s, d), c in zip(cadj, cut)], ws, True, inputs=dt)
    second = ops.edge_linear(x, [(s[c:], d[c:]) for (s, d), c in zip(cadj, cut)], ws, True, inputs=dt)
    parts, a, b = [], 0, 0
    for (s, _), c in zip(cadj, cut):
        parts += [first[a: a + c], second[b: b + s.numel() - c]]
        a, b = a + c, b + s.numel() - c
    assert torch.equal(torch.cat(parts), whole)
    # the edges of types 0 and 3 swapped between the types' lists (with the weights): other positions, same rows
    swapped = ops.edge_linear(x, [cadj[3], cadj[1], cadj[2], cadj[0]], [ws[3], ws[1], ws[2], ws[0]], True, inputs=dt)
    e = [int(s.numel()) for s, _ in cadj]
    assert torch.equal(swapped[: e[3]], whole[e[0] + e[1] + e[2]:])
    assert torch.equal(swapped[e[3] + e[1] + e[2]:], whole[: e[0]])


# ---------------------------------------------------------------------------------------------------------------------
# the layer: edge form and table form
# ---------------------------------------------------------------------------------------------------------------------
def _layer_under_mlp(key, dt, seed, pna=False):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    form, hidden, reduce, use_dst = key
    layer, x, adj = MC.layer_case(form, hidden, reduce, use_dst, seed, pna=pna)
    edges = sum(int(s.shape[0]) for s, _ in adj)
    assert L._prefer_edge_path(edges, x.shape[0], len(adj), hidden, hidden) == (form == "edge")
    weights = layer.export_weights()
    delta = 1.5 if pna else None
    exact, rounded = MC.mlp64(x, adj, weights, pna_delta=delta), MC.mlp64(x, adj, weights, dt=dt, pna_delta=delta)
    layer = layer.cuda()
    xg, adjg = x.cuda(), _cuda_adj(adj)
    with torch.no_grad():
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            got, since = _launches(lambda: MC.run_layer(layer, xg, adjg))
        assert ptgnn_amd.get_matrix_inputs() is torch.float32 and ptgnn_amd.mlp_inputs(xg) is torch.float32
    family = "half_linear" if form == "table" else ("edge16_dst" if use_dst else "edge16")
    assert since.get(family) == 1 and [f for f in HALF_FAMILIES if f in since] == [family], since
    assert not [f for f in FP32_EDGE_FAMILIES if f in since], since
    return got, rounded, exact, since


@DTYPES
@pytest.mark.parametrize("key", list(MC.LAYER_SEEDS), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{'dst' if k[3] else 'src'}")
def test_layer_takes_the_16_bit_message_gemm_with_the_flag(dt, key):
    form, hidden, _, use_dst = key
    got, rounded, exact, since = _layer_under_mlp(key, dt, MC.LAYER_SEEDS[key])
    if form == "edge" and hidden == 64:
        assert since.get("k_gather_update") == 1, since          # aggregation, LayerNorm and update: still ONE launch
    if form == "table":
        # the table is the only Linear that may round: the dense update stays ONE fp32 launch (its own, or the fused
        # aggregation + update)
        assert sum(since.get(f, 0) for f in FP32_LINEAR_FAMILIES + ("k_gather_update",)) == 1, since
    MC.check(got, rounded, exact, f"layer {key} {C.IDS[dt]}")


@DTYPES
@pytest.mark.parametrize("form", ["edge", "table"])
def test_pna_layer_takes_the_16_bit_message_gemm_with_the_flag(dt, form):
    got, rounded, exact, since = _layer_under_mlp((form, 64, "pna", True), dt, MC.PNA_SEEDS[form], pna=True)
    assert since.get("pna_aggregate") == 1, since
    MC.check(got, rounded, exact, f"PNA layer {form} {C.IDS[dt]}")


# ---------------------------------------------------------------------------------------------------------------------
# opt-in is opt-in
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("form", ["edge", "table"])
def test_settings_without_the_flag_leave_the_layer_at_its_fp32_bits(dt, form):
    import ptgnn_amd
    key = (form, 64, "sum", True)
    layer, x, adj = MC.layer_case(*key, MC.LAYER_SEEDS[key])
    layer, xg, adjg = layer.cuda(), x.cuda(), _cuda_adj(adj)
    with torch.no_grad():
        default = MC.run_layer(layer, xg, adjg)
        with ptgnn_amd.matrix_inputs(dt):
            plain, since = _launches(lambda: MC.run_layer(layer, xg, adjg))
        assert torch.equal(plain, default) and not [f for f in HALF_FAMILIES if f in since], since
        with ptgnn_amd.matrix_inputs(dt, edge_gemm=True, training=True):
            others, since = _launches(lambda: MC.run_layer(layer, xg, adjg))
        assert torch.equal(others, default) and not [f for f in HALF_FAMILIES if f in since], since
        with ptgnn_amd.matrix_inputs(torch.float32, mlp=True):
            assert torch.equal(MC.run_layer(layer, xg, adjg), default)


@DTYPES
def test_what_the_flag_does_not_cover_keeps_its_fp32_bits(dt):
    """Under `mlp=True`: a width that is no multiple of 32, one edge type in the edge form, a deep edge MLP, edge
    features and a call that needs gradients all equal the default output bit for bit, with no 16-bit launch."""
    import ptgnn_amd
    from ptgnn_amd import layers as L

    def both(layer, x, adj, feats=None, grad=False):
        layer, xg, adjg = layer.cuda(), x.cuda(), _cuda_adj(adj)
        feats = None if feats is None else [f.cuda() for f in feats]
        with torch.set_grad_enabled(grad):
            default = MC.run_layer(layer, xg, adjg, feats)
            with ptgnn_amd.matrix_inputs(dt, mlp=True):
                got, since = _launches(lambda: MC.run_layer(layer, xg, adjg, feats))
        assert torch.equal(got, default) and not [f for f in HALF_FAMILIES if f in since], since
        return got

    n = MC.N_NODES
    g = torch.Generator().manual_seed(8700)
    torch.manual_seed(8701)
    # widths that are no multiple of 32: 48 state columns in the table form, 48 message columns in the edge form
    x, adj = torch.randn(n, 48, generator=g), MC.adjacency(n, MC.FORMS["table"], 8702)
    both(L.MlpMessagePassingLayer(48, 48, 48, len(adj), "sum").eval(), x, adj)
    x, adj = torch.randn(n, 64, generator=g), MC.adjacency(n, MC.UNIT_ROWS, 8704)
    assert L._prefer_edge_path(sum(MC.UNIT_ROWS), n, len(adj), 64, 48)
    both(L.MlpMessagePassingLayer(64, 64, 48, len(adj), "sum").eval(), x, adj)
    both(L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum", mlp_hidden_layers=1).eval(), x, adj)      # deep edge MLP
    feats = [torch.randn(int(s.shape[0]), 8, generator=g) for s, _ in adj]
    both(L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum", features_dimension=8).eval(), x, adj, feats)
    got = both(L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum").eval(), x, adj, grad=True)          # needs gradients
    assert got.requires_grad


@DTYPES
def test_single_edge_type_in_the_edge_form_runs_fp32(dt):
    """ops level (the layer takes the table form for T = 1): one edge type is declined by the entry's shape predicate,
    the call runs the fp32 launch, silently -- as a message width of 36 does."""
    from ptgnn_amd import ops
    g = torch.Generator().manual_seed(8800)
    x = torch.randn(MC.N_NODES, 64, generator=g).cuda()
    ws = [C.xavier(64, 128, g).cuda() for _ in range(3)]
    cadj = _cuda_adj(MC.adjacency(MC.N_NODES, (40, 0, 70), 8801))
    assert not ops.edge_linear16_dst_supported(64, 64, 1, dt)
    got, since = _launches(lambda: ops.edge_linear(x, cadj[:1], ws[:1], True, inputs=dt))
    assert not [f for f in HALF_FAMILIES if f in since] and [f for f in FP32_EDGE_FAMILIES if f in since], since
    assert torch.equal(got, ops.edge_linear(x, cadj[:1], ws[:1], True))
    w36 = [w[:36].contiguous() for w in ws]
    got, since = _launches(lambda: ops.edge_linear(x, cadj, w36, True, inputs=dt))
    assert not [f for f in HALF_FAMILIES if f in since] and [f for f in FP32_EDGE_FAMILIES if f in since], since
    assert torch.equal(got, ops.edge_linear(x, cadj, w36, True))


@DTYPES
def test_ggnn_layer_does_not_follow_the_mlp_flag(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(8900)
    layer = L.GatedMessagePassingLayer(64, 64, 8, "sum").eval().cuda()
    x = torch.randn(300, 64, generator=torch.Generator().manual_seed(8901)).cuda()
    adj = _cuda_adj(C.random_adjacency(300, (25,) * 8, 8902))
    with torch.no_grad():
        with ptgnn_amd.matrix_inputs(dt):
            plain = MC.run_layer(layer, x, adj)
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            flagged, since = _launches(lambda: MC.run_layer(layer, x, adj))
    assert torch.equal(flagged, plain) and "edge16_dst" not in since, since


# ---------------------------------------------------------------------------------------------------------------------
# the entry's argument checks with real device operands (nothing here is out of range; nothing is meant to fault)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_and_leaves_msg_untouched():
    from ptgnn_amd import _lib, ops
    lib = _lib.load()
    n, h, m, T = 50, 64, 64, 3
    g = torch.Generator().manual_seed(9000)
    x = torch.randn(n, h, generator=g).cuda()
    w16 = torch.stack([C.xavier(m, 2 * h, g) for _ in range(T)]).to(torch.bfloat16).cuda()
    cadj = _cuda_adj(MC.adjacency(n, (40, 0, 70), 9001))
    counts = [int(s.shape[0]) for s, _ in cadj]
    msg = torch.full((sum(counts), m), 7.0, device="cuda")
    Ptr, Cnt = ctypes.c_void_p * T, ctypes.c_int64 * T
    sp = Ptr(*[s.data_ptr() if s.numel() else None for s, _ in cadj])
    dp = Ptr(*[d.data_ptr() if d.numel() else None for _, d in cadj])

    def call(x_ptr=x.data_ptr(), h_=h, m_=m, dtype=1, cnt=counts, dst=dp, w=w16.data_ptr(), ld_msg=None):
        rc = lib.ptgnn_amd_edge_dst_linear16(x_ptr, h, n, h_, ctypes.cast(sp, ctypes.c_void_p),
                                             ctypes.cast(dst, ctypes.c_void_p) if dst is not None else None,
                                             ctypes.cast(Cnt(*cnt), ctypes.c_void_p), w, T, m_, 0, dtype,
                                             msg.data_ptr(), m_ if ld_msg is None else ld_msg, None)
        return rc, lib.ptgnn_amd_last_error().decode()

    before = ops.launch_counts(edge16=True, edge16_dst=True)
    for kwargs, code, word in (({"x_ptr": None}, EINVAL, "null"), ({"w": None}, EINVAL, "null"),
                               ({"dtype": 0}, EINVAL, "dtype"), ({"dtype": 3}, EINVAL, "dtype"),
                               ({"cnt": [40, -1, 70]}, EINVAL, "negative"), ({"dst": None}, EINVAL, "target ids"),
                               ({"dst": Ptr(dp[0], None, None)}, EINVAL, "type 2"),
                               ({"h_": 48}, EUNSUPPORTED, "state_dim=48"), ({"m_": 36}, EUNSUPPORTED, "msg_dim=36")):
        rc, text = call(**kwargs)
        assert rc == code and text.startswith("edge_linear16: dst:") and word in text, (kwargs, rc, text)
    torch.cuda.synchronize()
    assert ops.launches_since(before) == {} and bool((msg == 7.0).all())              # nothing ran, msg untouched
    rc, _ = call(cnt=[0, 0, 0])                                                       # zero edges: no launch
    assert rc == 0 and ops.launches_since(before) == {} and bool((msg == 7.0).all())
    empty = [(torch.empty(0, dtype=torch.int64, device="cuda"),) * 2] * T
    ws = [torch.zeros(m, 2 * h, device="cuda")] * T
    got, since = _launches(lambda: ops.edge_linear(x, empty, ws, True, inputs=torch.bfloat16))
    assert got.shape == (0, m) and since == {}, since
    rc, _ = call()                                                                    # and the good call is taken
    assert rc == 0 and ops.launches_since(before) == {"edge16_dst": 1}
    want = ops.edge_linear(x, cadj, [w.float() for w in w16], True, inputs=torch.bfloat16)
    assert torch.equal(msg, want)
    with pytest.raises(_lib.PtgnnAmdError):
        ops.edge_linear(x, cadj, [w.float() for w in w16], True, inputs=torch.bfloat16, rounded=w16[:2])
    with pytest.raises(_lib.PtgnnAmdError, match="16-bit inputs"):
        ops.edge_linear(x, cadj, [w.float() for w in w16], True, inputs=torch.bfloat16, dropout=(1, 0.5, 7))
