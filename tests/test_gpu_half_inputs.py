"""The opt-in 16-bit matrix inputs on the MI355X: csrc/half_gemm.hip through `ops.linear` / `ops.gru_cell` /
`ops.aggregate_gru` (`inputs=`) and through the GGNN layer's inference routes under `ptgnn_amd.matrix_inputs`.

Reference: float64 on the ROUNDED operands; bar: TOL * max(1, |want|inf) (tests/half_cases.py says why that bar holds
for 16-bit operands, and why the layer tests take the aggregate the route rounded).  Every numeric test first asserts,
from the two float64 references alone, that rounding moves the result by at least 20 bars, and then that the kernel's
result is within one bar of the rounded reference and at least `gap - bar` from the exact one."""
import pytest
import torch

import half_cases as C

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
HALF_FAMILIES = ("half_linear", "half_gru")
FP32_GRU_FAMILIES = ("k_stream_gru", "k_gru", "k_stream_gru_ring")


def _launches(fn):
    """(result of fn, {family: launches it made}) over the GEMM and the half families."""
    from ptgnn_amd import ops
    before = ops.launch_counts(half=True)
    out = fn()
    return out, ops.launches_since(before)


def _check(got, rounded, exact, what):
    """The precondition on the inputs, then the two assertions on the result."""
    bar = C.bar(rounded)
    gap = C.err(exact, rounded)
    e, e_exact = C.err(got, rounded), C.err(got, exact)
    print(f"  {what}: bar {bar:.3e} gap {gap:.3e} |got - rounded| {e:.3e} |got - exact| {e_exact:.3e}")
    assert gap >= C.MARGIN * bar, f"{what}: inputs do not tell the references apart ({gap:.3e} < 20 x {bar:.3e})"
    assert e <= bar, f"{what}: {e:.3e} > {bar:.3e}"
    assert e_exact >= gap - bar, what


def _cuda(*ts):
    return [t.cuda() if t is not None else None for t in ts]


# ---------------------------------------------------------------------------------------------------------------------
# exact integer data: the fragment maps, the k-step, row and column tails
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_linear_is_exact_on_integer_data(dt):
    from ptgnn_amd import ops
    for k in (32, 64, 96):
        for n_out in (32, 96, 160):
            x_all, w, b = C.integer_case(129, k, n_out, 9000 + k + n_out)
            want_all = x_all @ w.t()                     # integers below 2^24: exact in fp32 in any order
            xg, wg, bg = _cuda(x_all, w, b)
            for rows in (1, 31, 32, 33, 127, 129):
                for bias in (None, bg):
                    got, since = _launches(lambda: ops.linear(xg[:rows], wg, bias, inputs=dt))
                    assert since == {"half_linear": 1}, since
                    want = want_all[:rows] + (b if bias is not None else 0)
                    assert torch.equal(got.cpu(), want), (C.IDS[dt], rows, k, n_out, bias is not None)


@DTYPES
def test_gru_gate_gemms_are_exact_on_integer_data(dt):
    """The GRU's r and z chains run over K = M + H and its n gate keeps two accumulators: with integer operands and
    zero biases the pre-activations are integers, so float64 on them differs from the kernel by the gate math alone."""
    from ptgnn_amd import ops
    g = torch.Generator().manual_seed(9100)
    for m, hd in ((32, 32), (96, 64), (64, 96)):
        rows = 129
        a = torch.randint(-2, 3, (rows, m), generator=g).float()
        h = torch.randint(-2, 3, (rows, hd), generator=g).float()
        w_ih = torch.randint(-1, 2, (3 * hd, m), generator=g).float() * 0.125
        w_hh = torch.randint(-1, 2, (3 * hd, hd), generator=g).float() * 0.125
        zero = torch.zeros(3 * hd)
        want = C.gru64(a, h, w_ih, w_hh, zero, zero)          # no rounding anywhere: every operand is exact in 16 bits
        got = ops.gru_cell(*_cuda(a, h, w_ih, w_hh, zero, zero), inputs=dt)
        assert C.err(got, want) <= C.bar(want), (C.IDS[dt], m, hd, C.err(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# random data against float64 on the rounded operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linear_case():
    g = torch.Generator().manual_seed(9200)
    x, w, b = torch.randn(300, 128, generator=g), C.xavier(384, 128, g), torch.randn(384, generator=g) * 0.1
    return x, w, b, _cuda(x, w, b)


@DTYPES
@pytest.mark.parametrize("act", [None, "tanh"])
def test_linear_matches_float64_on_the_rounded_operands(linear_case, dt, act):
    from ptgnn_amd import ops
    x, w, b, (xg, wg, bg) = linear_case
    got, since = _launches(lambda: ops.linear(xg, wg, bg, act=act, inputs=dt))
    assert since == {"half_linear": 1}, since
    _check(got, C.linear64(x, w, b, act, dt), C.linear64(x, w, b, act), f"linear {C.IDS[dt]} act={act}")
    given = ops.linear(xg, wg, bg, act=act, inputs=dt, rounded=wg.to(dt))     # the caller's rounded copy: same bits
    assert torch.equal(given, got)


@pytest.fixture(scope="module")
def gru_cases():
    """(m, hd) -> 300-row case; the row counts of the tests are prefixes of it.  The seeds are ones at which the two
    float64 references are at least 24 bars apart for fp16 at every row count, the single first row included (with
    other seeds a lone row sits at 17 - 21 bars, around the precondition's 20); bf16 is above 100 everywhere."""
    seeds = {(64, 64): 9316, (128, 64): 9300, (64, 128): 9381, (128, 128): 9505}
    return {key: C.gru_case(300, *key, seed) for key, seed in seeds.items()}


@DTYPES
@pytest.mark.parametrize("m,hd", [(64, 64), (128, 64), (64, 128), (128, 128)])
@pytest.mark.parametrize("rows", [1, 33, 300])
def test_gru_cell_matches_float64_on_the_rounded_operands(gru_cases, dt, m, hd, rows):
    from ptgnn_amd import ops
    a, h, *params = gru_cases[(m, hd)]
    a, h = a[:rows], h[:rows]
    got, since = _launches(lambda: ops.gru_cell(*_cuda(a, h, *params), inputs=dt))
    assert since == {"half_gru": 1}, since
    _check(got, C.gru64(a, h, *params, dt=dt), C.gru64(a, h, *params), f"gru {C.IDS[dt]} rows={rows} m={m} hd={hd}")


@DTYPES
@pytest.mark.parametrize("m,hd,rows,seed", [(96, 96, 129, 9801), (256, 256, 33, 9801), (32, 160, 65, 9802)])
def test_gru_cell_at_widths_outside_the_weight_stationary_kernel(dt, m, hd, rows, seed):
    """M, H in {64, 128} run the weight-stationary kernel; every other supported width the per-wave one (hd % 64 == 0:
    two feature tiles per wave, else one).  Seeds: the references are at least 24 bars apart for fp16."""
    from ptgnn_amd import ops
    a, h, *params = C.gru_case(rows, m, hd, seed)
    got, since = _launches(lambda: ops.gru_cell(*_cuda(a, h, *params), inputs=dt))
    assert since == {"half_gru": 1}, since
    _check(got, C.gru64(a, h, *params, dt=dt), C.gru64(a, h, *params), f"gru {C.IDS[dt]} rows={rows} m={m} hd={hd}")


@DTYPES
@pytest.mark.parametrize("hd", [64, 128])
def test_the_two_gru_kernels_give_the_same_bits(dt, hd):
    """M = 64 runs the weight-stationary kernel; the same case with M padded to 96 by zero columns of `a` and W_ih runs
    the per-wave one (96 is outside {64, 128}).  The pad's k-steps add exact zeros to the r, z and i_n accumulators after
    the real `a` steps and before the h phase, so the chains -- and with the shared gate math the results -- are equal."""
    from ptgnn_amd import ops
    rows, m = 65, 64
    a, h, w_ih, w_hh, b_ih, b_hh = _cuda(*C.gru_case(rows, m, hd, 9950 + hd))
    a_pad = torch.cat([a, torch.zeros(rows, 32, device="cuda")], 1)
    w_ih_pad = torch.cat([w_ih, torch.zeros(3 * hd, 32, device="cuda")], 1)
    stationary, since = _launches(lambda: ops.gru_cell(a, h, w_ih, w_hh, b_ih, b_hh, inputs=dt))
    assert since == {"half_gru": 1}, since
    per_wave, since = _launches(lambda: ops.gru_cell(a_pad, h, w_ih_pad, w_hh, b_ih, b_hh, inputs=dt))
    assert since == {"half_gru": 1}, since
    assert torch.equal(per_wave, stationary), (C.IDS[dt], hd)


# ---------------------------------------------------------------------------------------------------------------------
# strides, row offsets, row independence
# ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_padded_rows_output_slices_and_row_offsets(gru_cases, linear_case, dt):
    from ptgnn_amd import ops
    nan = float("nan")
    # Linear: ld_x > k with NaN in the pad columns, rows from row 32 on, output into a column slice
    x, w, b, (xg, wg, bg) = linear_case
    plain = ops.linear(xg, wg, bg, inputs=dt)
    xpad = torch.full((300, 128 + 8), nan, device="cuda")
    xpad[:, :128] = xg
    ybuf = torch.full((300, 384 + 4), -7.0, device="cuda")
    got, since = _launches(lambda: ops.linear(xpad[32:, :128], wg, bg, out=ybuf[32:, :384], inputs=dt))
    assert since == {"half_linear": 1}, since
    assert got.data_ptr() == ybuf[32:].data_ptr() and torch.equal(ybuf[32:, :384], plain[32:])
    assert bool((ybuf[:32] == -7.0).all()) and bool((ybuf[:, 384:] == -7.0).all())
    # GRU: padded a and h, `out` = the right half of a [rows, 2 hd] buffer whose left half must come back untouched
    a, h, *params = gru_cases[(128, 64)]
    ag, hg, *pg = _cuda(a, h, *params)
    plain = ops.gru_cell(ag, hg, *pg, inputs=dt)
    apad = torch.full((300, 128 + 4), nan, device="cuda")
    hpad = torch.full((300, 64 + 12), nan, device="cuda")
    apad[:, :128], hpad[:, :64] = ag, hg
    left = torch.randn(300, 64, generator=torch.Generator().manual_seed(9400)).cuda()
    buf = torch.cat([left, torch.full((300, 64), nan, device="cuda")], dim=1)
    got, since = _launches(lambda: ops.gru_cell(apad[:, :128], hpad[:, :64], *pg, out=buf[:, 64:], inputs=dt))
    assert since == {"half_gru": 1}, since
    assert torch.equal(buf[:, 64:], plain) and torch.equal(buf[:, :64], left)
    _check(buf[:, 64:], C.gru64(a, h, *params, dt=dt), C.gru64(a, h, *params), f"gru into a slice {C.IDS[dt]}")
    # a view that starts at row 32, written into rows 32.. of the buffer
    buf2 = torch.cat([left, torch.full((300, 64), -7.0, device="cuda")], dim=1)
    ops.gru_cell(apad[32:, :128], hpad[32:, :64], *pg, out=buf2[32:, 64:], inputs=dt)
    assert torch.equal(buf2[32:, 64:], plain[32:]) and bool((buf2[:32, 64:] == -7.0).all())
    assert torch.equal(buf2[:, :64], left)


@DTYPES
def test_rows_do_not_depend_on_the_launch_they_are_in(gru_cases, linear_case, dt):
    from ptgnn_amd import ops
    cuts = ((0, 96), (96, 224), (224, 300))
    for key in gru_cases:
        ag, hg, *pg = _cuda(*gru_cases[key])
        whole = ops.gru_cell(ag, hg, *pg, inputs=dt)
        parts = torch.cat([ops.gru_cell(ag[lo:hi], hg[lo:hi], *pg, inputs=dt) for lo, hi in cuts])
        assert torch.equal(parts, whole), (C.IDS[dt], key)
        for r in (0, 31, 45, 299):                       # and not on the row's position: row r alone
            assert torch.equal(ops.gru_cell(ag[r:r + 1].clone(), hg[r:r + 1].clone(), *pg, inputs=dt), whole[r:r + 1])
    _, _, _, (xg, wg, bg) = linear_case
    whole = ops.linear(xg, wg, bg, act="tanh", inputs=dt)
    parts = torch.cat([ops.linear(xg[lo:hi], wg, bg, act="tanh", inputs=dt) for lo, hi in cuts])
    assert torch.equal(parts, whole)
    assert torch.equal(ops.linear(xg[45:46].clone(), wg, bg, act="tanh", inputs=dt), whole[45:46])
    assert ops.linear(xg[:0], wg, bg, inputs=dt).shape == (0, 384)                    # no rows: no launch
    assert ops.gru_cell(ag[:0], hg[:0], *pg, inputs=dt).shape == (0, hg.shape[1])


@pytest.mark.parametrize("m,hd", [(64, 128), (128, 64)])
def test_more_row_panels_than_workgroups(m, hd):
    """The weight-stationary GRU walks its 32-row (H = 128) or 64-row (H = 64) panels workgroup-strided through two LDS
    buffers: with 2 x CUs panels and a 37-row tail every workgroup makes two or three trips.  Against float64, and
    bitwise against single-trip launches over 4096-row pieces."""
    from ptgnn_amd import ops
    dt = torch.bfloat16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * cus * (32 if hd == 128 else 64) + 37
    a, h, *params = C.gru_case(rows, m, hd, 9900 + hd)
    ag, hg, *pg = _cuda(a, h, *params)
    got = ops.gru_cell(ag, hg, *pg, inputs=dt)
    _check(got, C.gru64(a, h, *params, dt=dt), C.gru64(a, h, *params), f"gru rows={rows} m={m} hd={hd}")
    parts = torch.cat([ops.gru_cell(ag[lo:lo + 4096], hg[lo:lo + 4096], *pg, inputs=dt) for lo in range(0, rows, 4096)])
    assert torch.equal(parts, got)


# ---------------------------------------------------------------------------------------------------------------------
# the GGNN layer's routes
# ---------------------------------------------------------------------------------------------------------------------
def _layer_case(form):
    """(layer, x, adjacency): table form = 400 nodes, 3 types, 1200 edges; edge form = 300 nodes, 8 types, 200 edges."""
    from ptgnn_amd import layers as L
    n, counts, seed = (400, (600, 400, 200), 9500) if form == "table" else (300, (25,) * 8, 9600)
    torch.manual_seed(seed)
    layer = L.GatedMessagePassingLayer(64, 64, len(counts), "sum").eval()
    x = torch.randn(n, 64, generator=torch.Generator().manual_seed(seed + 1))
    adj = C.random_adjacency(n, counts, seed + 2)
    assert L._prefer_edge_path(sum(counts), n, len(counts), 64, 64) == (form == "edge")
    return layer, x, adj


def _run(layer, x, adj):
    from ptgnn_amd import ops
    ops.clear_plan_cache()
    feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    return layer(x, adj, None, {}, {}, feats)


@pytest.mark.parametrize("form", ["table", "edge"])
def test_layer_inference_routes_take_the_half_kernels(monkeypatch, form):
    import ptgnn_amd
    from ptgnn_amd import ops
    dt = torch.bfloat16
    layer, x, adj = _layer_case(form)
    weights = layer.export_weights()
    linear_dt = dt if form == "table" else None                    # the grouped per-edge GEMM stays fp32
    exact, _ = C.ggnn64(x, adj, weights)
    rounded_f64, agg64 = C.ggnn64(x, adj, weights, linear_dt=linear_dt, gru_dt=dt)
    assert C.err(exact, rounded_f64) >= C.MARGIN * C.bar(rounded_f64)          # from the references alone
    layer = layer.cuda()
    xg, adjg = x.cuda(), [(s.cuda(), d.cuda()) for s, d in adj]
    with torch.no_grad():
        default, since = _launches(lambda: _run(layer, xg, adjg))
        assert not [f for f in HALF_FAMILIES if f in since], since              # default mode: no half family
        assert [f for f in FP32_GRU_FAMILIES if f in since], since
        with ptgnn_amd.matrix_inputs(dt), C.captured(monkeypatch, ops, "gather_reduce") as seen:
            got, since = _launches(lambda: _run(layer, xg, adjg))
        assert ptgnn_amd.get_matrix_inputs() is torch.float32
    assert since.get("half_gru") == 1 and not [f for f in FP32_GRU_FAMILIES if f in since], since
    assert since.get("half_linear", 0) == (1 if form == "table" else 0), since
    assert len(seen) == 1
    e_agg = C.err(seen[0], agg64)
    print(f"  {form}: aggregate |got - float64| {e_agg:.3e} (bar {C.bar(agg64):.3e})")
    assert e_agg <= C.bar(agg64)
    want, _ = C.ggnn64(x, adj, weights, linear_dt=linear_dt, gru_dt=dt, agg=seen[0])
    _check(got, want, exact, f"layer {form} form")
    assert C.err(default, exact) <= C.bar(exact)


def test_edge_feature_inference_route_takes_the_half_gru(monkeypatch):
    """With per-edge features the messages come from the grouped GEMM (fp32 under every setting) and only the GRU cell
    follows the setting: its result against float64 on the aggregate that route produced, rounded."""
    import ptgnn_amd
    from ptgnn_amd import layers as L, ops
    dt = torch.bfloat16
    torch.manual_seed(9650)
    layer = L.GatedMessagePassingLayer(64, 64, 3, "sum", edge_feature_dimension=8).eval()
    w = layer.export_weights()
    x = torch.randn(300, 64, generator=torch.Generator().manual_seed(9651))
    adj = C.random_adjacency(300, (400, 300, 200), 9652)
    g = torch.Generator().manual_seed(9653)
    feats = [torch.randn(int(s.shape[0]), 8, generator=g).cuda() for s, _ in adj]
    layer = layer.cuda()
    xg, adjg = x.cuda(), [(s.cuda(), d.cuda()) for s, d in adj]
    ops.clear_plan_cache()
    with torch.no_grad():
        default, since = _launches(lambda: layer(xg, adjg, None, {}, {}, feats))
        assert not [f for f in HALF_FAMILIES if f in since], since
        with ptgnn_amd.matrix_inputs(dt), C.captured(monkeypatch, ops, "gather_reduce") as seen:
            got, since = _launches(lambda: layer(xg, adjg, None, {}, {}, feats))
    assert since.get("half_gru") == 1 and "half_linear" not in since, since
    assert not [f for f in FP32_GRU_FAMILIES if f in since] and len(seen) == 1
    gru = (w["w_ih"], w["w_hh"], w["b_ih"], w["b_hh"])
    _check(got, C.gru64(seen[0], x, *gru, dt=dt), C.gru64(seen[0], x, *gru), "edge-feature route")
    assert C.err(default, C.gru64(seen[0], x, *gru)) <= C.bar(default)


def test_aggregate_gru_row_ranges_give_the_bits_of_one_launch(monkeypatch):
    import ptgnn_amd
    from ptgnn_amd import ops
    layer, x, adj = _layer_case("table")
    layer = layer.cuda()
    xg, adjg = x.cuda(), [(s.cuda(), d.cuda()) for s, d in adj]
    with torch.no_grad(), ptgnn_amd.matrix_inputs(torch.bfloat16):
        one = _run(layer, xg, adjg)
        monkeypatch.setattr(ops, "AGG_PIPELINE", 3)
        monkeypatch.setattr(ops, "AGG_PIPELINE_MIN_ROWS", 0)
        ranges, since = _launches(lambda: _run(layer, xg, adjg))
    torch.cuda.synchronize()
    assert since.get("half_gru") == 3, since
    assert torch.equal(ranges, one)


def test_bf16_states_under_autocast_take_the_half_route_after_the_upcast():
    """The bar of test_amp_dtypes_are_upcast_like_the_reference_aggregation (tests/test_gpu_parity.py): 8e-3 for bf16,
    scaled by max(1, |want|inf), against the exact layer on the same (rounded) input states."""
    import ptgnn_amd
    layer, x, adj = _layer_case("table")
    x_lo = x.to(torch.bfloat16)
    want, _ = C.ggnn64(x_lo.float(), adj, layer.export_weights())
    layer = layer.cuda()
    adjg = [(s.cuda(), d.cuda()) for s, d in adj]
    ptgnn_amd.set_matrix_inputs("autocast")
    try:
        with torch.no_grad():
            outside, since_outside = _launches(lambda: _run(layer, x_lo.cuda(), adjg))       # no autocast region: fp32
            with torch.autocast("cuda", dtype=torch.bfloat16):
                got, since = _launches(lambda: _run(layer, x_lo.cuda(), adjg))
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    assert not [f for f in HALF_FAMILIES if f in since_outside], since_outside
    assert since.get("half_gru") == 1 and since.get("half_linear") == 1, since
    assert got.dtype == torch.bfloat16 and outside.dtype == torch.bfloat16
    e = C.err(got.float(), want)
    print(f"  bf16 states: |got - exact| {e:.3e}, bar {8e-3 * max(1.0, float(want.abs().max())):.3e}")
    assert e <= 8e-3 * max(1.0, float(want.abs().max()))


def test_training_ignores_the_setting():
    import ptgnn_amd
    layer, x, adj = _layer_case("table")
    layer = layer.cuda().train()
    xg, adjg = x.cuda(), [(s.cuda(), d.cuda()) for s, d in adj]
    default = _run(layer, xg, adjg)
    with ptgnn_amd.matrix_inputs(torch.bfloat16):
        got, since = _launches(lambda: _run(layer, xg, adjg))
    assert got.requires_grad and not [f for f in HALF_FAMILIES if f in since], since
    assert torch.equal(got, default)


def test_unsupported_width_runs_the_fp32_kernels():
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(9700)
    layer = L.GatedMessagePassingLayer(30, 30, 3, "sum").eval().cuda()
    xg = torch.randn(200, 30, generator=torch.Generator().manual_seed(9701)).cuda()
    adjg = [(s.cuda(), d.cuda()) for s, d in C.random_adjacency(200, (300, 200, 100), 9702)]
    with torch.no_grad():
        default = _run(layer, xg, adjg)
        with ptgnn_amd.matrix_inputs(torch.bfloat16):
            got, since = _launches(lambda: _run(layer, xg, adjg))
    assert not [f for f in HALF_FAMILIES if f in since] and [f for f in FP32_GRU_FAMILIES if f in since], since
    assert torch.equal(got, default)
