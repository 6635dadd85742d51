"""Every dispatch path of the CSR aggregation kernels at its thresholds, against float64 and the serial fp32 oracle.

The graphs come from tests/agg_paths.py: destination rows at in-degrees 0 .. 17, 255 .. 258, 1023 .. 1025, 2047 .. 2049,
3073 and 4097, hubs at row 0, at row N-1 and on two adjacent rows that share a 1024-slot chunk, a source with > 2048
out-edges of one type (a hub row of the backward plan), and messages from small integer sets with both signed zeros.
Each test first asserts that its inputs reach the path it is about (hub list non-empty, the degree bins, plan size
against 2^19 / 2^21, float4 eligibility), so a moved threshold fails here instead of silently testing the main path.

Bars:
  * rows of in-degree <= 2048, sum / mean: bit-identical to oracle.scatter_ref (serial fp32 fold in message order);
  * hub rows, sum / mean: |got - float64| <= 5e-6 (1 + mass), bitwise repeatable, tickets back to zero;
  * max / min: value bits (signed zeros included) and arg equal to torch_scatter's serial fold (the earliest message
    wins a tie) on every row;
  * PNA / EGC outputs and all gradients: the attributed bar (agg_paths.attributed_ok).
The side-stream and caller-stream hub launches read their environment switches once per process: they run in a child
process (tests/agg_paths_side_check.py)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import agg_paths as AP
from helpers import to_cuda_adj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class Case:
    """A spectrum graph with its plan and its messages' (src, dst, type) in message order."""

    def __init__(self, num_types):
        from ptgnn_amd import ops
        self.sp = AP.spectrum_graph(num_types=num_types)
        self.N, self.E, self.T = self.sp.num_nodes, self.sp.num_edges, num_types
        self.src, self.dst, self.typ = self.sp.src_dst_type()
        self.deg = self.sp.deg
        self.small = self.deg <= AP.HUB_THRESHOLD
        self.adj = to_cuda_adj(self.sp.adj)
        self.plan = ops.build_plan(self.adj, self.N)
        self.perm = self.plan.perm[: self.E].cpu().long()

    def assert_hub_plan(self, plan=None):
        from ptgnn_amd import ops
        plan = plan or self.plan
        assert ops.HUB_THRESHOLD == AP.HUB_THRESHOLD == 2048
        assert plan.may_have_hubs() and int(plan.hub_count.reshape(-1)[0]) > 0
        assert plan.num_edges < (1 << 19)                   # the fused hub walk, below the side streams' 2^21

    def table_msgs(self, y, M, yd=None):
        m = y.view(self.N, self.T, M)[self.src, self.typ]
        if yd is not None:
            m = m + yd.view(self.N, self.T, M)[self.dst, self.typ]
        return m


_CASES = {}


def case(num_types):
    _need_gpu()
    if num_types not in _CASES:
        _CASES[num_types] = Case(num_types)
    return _CASES[num_types]


def values(rows, cols, reduce, seed):
    """Tie-heavy integers (signed zeros) for max / min, normal floats (order-sensitive sums) for sum / mean."""
    if reduce in ("max", "min"):
        return AP.tie_values(rows, cols, seed)
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def slot_to_edge(arg, perm, E):
    arg = arg.cpu().long()
    return torch.where(arg >= 0, perm[arg.clamp(min=0)], torch.full_like(arg, E))


def check_reduce(c, got, msgs, reduce, arg=None, rows=None, what=""):
    """`got` [N, M] (CPU) of `reduce` over msgs [E, M] (message order) with the bars of the module docstring;
    `rows` = (lo, hi) restricts the check."""
    from oracle import scatter_ref
    lo, hi = rows or (0, c.N)
    sel = torch.zeros(c.N, dtype=torch.bool)
    sel[lo:hi] = True
    if reduce in ("max", "min"):
        want, want_arg = AP.first_winner(msgs, c.dst, c.N, reduce)
        bad = (got.view(I32) != want.view(I32)).any(1) & sel
        assert not bool(bad.any()), (what, "value bits", torch.nonzero(bad).flatten()[:8].tolist(),
                                     c.deg[bad][:8].tolist())
        if arg is not None:
            got_edge = slot_to_edge(arg, c.perm, c.E)
            bad = (got_edge != want_arg).any(1) & sel
            assert not bool(bad.any()), (what, "arg", torch.nonzero(bad).flatten()[:8].tolist(), c.deg[bad][:8].tolist())
        return
    want32 = scatter_ref.scatter(msgs, c.dst, dim=0, dim_size=c.N, reduce=reduce)
    small = c.small & sel
    bad = (got.view(I32) != want32.view(I32)).any(1) & small
    assert not bool(bad.any()), (what, "serial-order bits", torch.nonzero(bad).flatten()[:8].tolist(),
                                 c.deg[bad][:8].tolist())
    hub = ~c.small & sel
    if bool(hub.any()):
        m64 = msgs.double()
        want64 = scatter_ref.scatter(m64, c.dst, dim=0, dim_size=c.N, reduce=reduce)
        mass = scatter_ref.scatter(m64.abs(), c.dst, dim=0, dim_size=c.N, reduce=reduce)
        err = ((got.double() - want64).abs() / (1.0 + mass))[hub]
        assert float(err.max()) <= 5e-6, (what, "hub rows vs float64", float(err.max()))


REDUCES = ["sum", "mean", "max", "min"]
WIDTHS = [1, 3, 4, 60, 64, 65, 68, 128, 132, 255, 256, 260, 512, 516, 1028]


# ---------------------------------------------------------------------------------------------------------------------
# ops.gather_reduce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", WIDTHS)
@pytest.mark.parametrize("reduce", REDUCES)
def test_gather_reduce_edge_form_every_width(reduce, M):
    """Edge form (type_bits 0, col = perm): every lane geometry (VEC 4 / 1 x LPR 16 / 32 / 64 x CH 1 / 2 / 4, extra
    column blocks past 512 / 256); max / min with and without arg (the fused hub walk vs the dedicated hub launch)."""
    from ptgnn_amd import ops
    c = case(1)
    c.assert_hub_plan()
    msgs = values(c.E, M, reduce, seed=M)
    y = msgs.cuda()
    assert y.data_ptr() % 16 == 0                       # float4 rows exactly when M % 4 == 0
    out = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm)
    # caught: max / min without arg on hub rows (hub_chunks_body, fused and dedicated) returned the wrong signed zero
    check_reduce(c, out.cpu(), msgs, reduce, what=f"edge {reduce} M={M}")
    if reduce in ("max", "min"):
        out2, arg = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm, return_arg=True)
        check_reduce(c, out2.cpu(), msgs, reduce, arg=arg, what=f"edge {reduce} M={M} arg")
    else:
        again = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm)
        assert torch.equal(out.view(I32), again.view(I32)), "two runs differ"
    torch.cuda.synchronize()
    assert int(c.plan.hub_tickets(M).abs().sum()) == 0


@pytest.mark.parametrize("reduce", REDUCES)
def test_gather_reduce_unaligned_view_takes_the_scalar_path(reduce):
    from ptgnn_amd import ops
    c = case(1)
    big = values(c.E, 66, reduce, seed=66).cuda()
    y = big[:, 1:65]                                   # ld 66, 4-byte offset: VEC1 at M = 64
    assert y.data_ptr() % 16 != 0
    msgs = y.cpu().contiguous()
    res = ops.gather_reduce(y, c.plan, 64, reduce, type_bits=0, col=c.plan.perm, return_arg=reduce in ("max", "min"))
    out, arg = res if isinstance(res, tuple) else (res, None)
    check_reduce(c, out.cpu(), msgs, reduce, arg=arg, what=f"unaligned {reduce}")


@pytest.mark.parametrize("M", [3, 64, 65, 256, 512, 516])
@pytest.mark.parametrize("form", ["table3", "dst1", "dst3"])
@pytest.mark.parametrize("reduce", REDUCES)
def test_gather_reduce_table_and_destination_forms(reduce, form, M):
    """Table form with T = 3, and a destination term at T = 1 (the DST1 variant and, below 2^19 edges, the hub walk of
    its own instantiation) and T = 3 (per-slot destination term, groups of 4)."""
    from ptgnn_amd import ops
    T = 1 if form == "dst1" else 3
    c = case(T)
    c.assert_hub_plan()
    y = values(c.N, T * M, reduce, seed=M + 1)
    yd = values(c.N, T * M, reduce, seed=M + 2) if form != "table3" else None
    msgs = c.table_msgs(y, M, yd)
    for want_arg in ([False, True] if reduce in ("max", "min") else [False]):
        res = ops.gather_reduce(y.cuda(), c.plan, M, reduce, ydst=yd.cuda() if yd is not None else None,
                                return_arg=want_arg)
        out, arg = res if want_arg else (res, None)
        check_reduce(c, out.cpu(), msgs, reduce, arg=arg, what=f"{form} {reduce} M={M} arg={want_arg}")
    torch.cuda.synchronize()
    assert int(c.plan.hub_tickets(M).abs().sum()) == 0


def _ln_ref(agg, M, w, b):
    return F.layer_norm(F.gelu(agg), (M,), w.to(agg.dtype), b.to(agg.dtype), eps=1e-5)


@pytest.mark.parametrize("M,aligned", [(64, True), (256, True), (512, True), (255, False)])
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_gather_reduce_gelu_layernorm_epilogue(reduce, M, aligned):
    from oracle import scatter_ref
    from ptgnn_amd import ops
    c = case(1)
    c.assert_hub_plan()
    msgs = values(c.E, M, reduce, seed=M + 7)
    y = msgs.cuda()
    if not aligned:
        y = torch.zeros(c.E, M + 1, device="cuda")[:, 1:]
        y.copy_(msgs.cuda())
        assert y.data_ptr() % 16 != 0
    g = torch.Generator().manual_seed(3)
    w, b = torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g)
    out = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm, epilogue=ops.EPI_GELU_LAYERNORM,
                            ln_weight=w.cuda(), ln_bias=b.cuda())
    if reduce == "sum":
        a32 = scatter_ref.scatter(msgs, c.dst, dim=0, dim_size=c.N, reduce="sum")
        a64 = scatter_ref.scatter(msgs.double(), c.dst, dim=0, dim_size=c.N, reduce="sum")
    else:
        a32 = AP.first_winner(msgs, c.dst, c.N, "max")[0]
        a64 = a32.double()
    assert AP.attributed_ok(out, _ln_ref(a32, M, w, b), _ln_ref(a64, M, w, b))


@pytest.mark.parametrize("M,aligned", [(516, True), (1028, True), (257, False), (260, False)])
def test_gather_reduce_epilogue_past_its_limit_is_unsupported_and_writes_nothing(M, aligned):
    from ptgnn_amd import _lib, ops
    c = case(1)
    y = torch.randn(c.E, M + (0 if aligned else 1), device="cuda")
    if not aligned:
        y = y[:, 1:]
    out = torch.full((c.N, M), float("nan"), device="cuda")
    before = out.clone()
    with pytest.raises(_lib.PtgnnAmdError, match=r"code -2"):
        ops.gather_reduce(y, c.plan, M, "sum", type_bits=0, col=c.plan.perm, epilogue=ops.EPI_GELU_LAYERNORM,
                          ln_weight=torch.ones(M, device="cuda"), ln_bias=torch.zeros(M, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert torch.equal(out.view(I32), before.view(I32))


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_gather_reduce_row_ranges_around_hubs(reduce):
    """rows = (lo, hi): hub rows inside and outside the range (one range splits the adjacent hub pair); rows outside
    stay untouched."""
    from ptgnn_amd import ops
    c = case(1)
    c.assert_hub_plan()
    M = 64
    msgs = values(c.E, M, reduce, seed=17)
    y = msgs.cuda()
    r0, r1 = c.sp.shared_pair
    for lo, hi in [(0, 1), (1, c.N - 1), (r0 - 5, r0 + 1), (r1, c.N), (0, c.N)]:
        out = torch.full((c.N, M), float("nan"), device="cuda")
        ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm, out=out, rows=(lo, hi))
        got = out.cpu()
        check_reduce(c, got, msgs, reduce, rows=(lo, hi), what=f"rows {lo}:{hi}")
        outside = torch.ones(c.N, dtype=torch.bool)
        outside[lo:hi] = False
        assert bool(torch.isnan(got[outside]).all()), f"rows {lo}:{hi} wrote outside its range"
    torch.cuda.synchronize()
    assert int(c.plan.hub_tickets(M).abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# backward: scatter.gather_reduce (backward plan with a hub row, masked max / min) and segment_spread
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [64, 132])
@pytest.mark.parametrize("T,with_dst", [(1, False), (1, True), (3, False), (3, True)])
@pytest.mark.parametrize("reduce", REDUCES)
def test_gather_reduce_backward_against_float64_autograd(reduce, T, with_dst, M):
    from ptgnn_amd import scatter
    c = case(T)
    c.assert_hub_plan()
    bp = c.plan.backward_plan()
    c.assert_hub_plan(bp)                               # the hub source: gather_reduce(_masked) take their hub paths
    y = values(c.N, T * M, reduce, seed=M + 31)
    yd = values(c.N, T * M, reduce, seed=M + 32) if with_dst else None
    gout = torch.randn(c.N, M, generator=torch.Generator().manual_seed(5))
    yg = y.cuda().requires_grad_(True)
    ydg = yd.cuda().requires_grad_(True) if with_dst else None
    out = scatter.gather_reduce(yg, ydg, c.plan, M, reduce)
    (out * gout.cuda()).sum().backward()

    def ref(dtype):
        y_ = y.to(dtype).clone().requires_grad_(True)
        yd_ = yd.to(dtype).clone().requires_grad_(True) if with_dst else None
        o = AP.segment_ref(c.table_msgs(y_, M, yd_), c.dst, c.N, reduce)
        (o * gout.to(dtype)).sum().backward()
        return o, y_.grad, (yd_.grad if with_dst else None)

    o32, g32, gd32 = ref(torch.float32)
    o64, g64, gd64 = ref(torch.float64)
    assert AP.attributed_ok(out, o32, o64)
    sc = max(1.0, float(g64.abs().max()))
    assert AP.attributed_ok(yg.grad, g32, g64, scale=sc), "d ysrc"
    if with_dst:
        assert AP.attributed_ok(ydg.grad, gd32, gd64, scale=max(1.0, float(gd64.abs().max()))), "d ydst"


@pytest.mark.parametrize("D,view", [(64, False), (128, False), (256, False), (1, False), (65, False), (260, False),
                                    (64, True)])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_segment_spread_row_and_generic_kernels(reduce, D, view):
    """segment_reduce backward: the row kernel at 64 / 128 / 256, the generic kernel at every other width and for an
    unaligned view; with (max) and without (sum / mean) the arg."""
    from ptgnn_amd import scatter
    c = case(1)
    msgs = values(c.E, D, reduce, seed=D + 41)
    if view:
        big = torch.zeros(c.E, D + 1, device="cuda", requires_grad=True)
        with torch.no_grad():
            big[:, 1:] = msgs.cuda()
        leaf, m = big, big[:, 1:]
        assert m.data_ptr() % 16 != 0
    else:
        leaf = msgs.cuda().requires_grad_(True)
        m = leaf
    gout = torch.randn(c.N, D, generator=torch.Generator().manual_seed(6))
    out = scatter.segment_reduce(m, c.plan, reduce)
    (out * gout.cuda()).sum().backward()
    grad = leaf.grad[:, 1:] if view else leaf.grad

    def ref(dtype):
        m_ = msgs.to(dtype).clone().requires_grad_(True)
        o = AP.segment_ref(m_, c.dst, c.N, reduce)
        (o * gout.to(dtype)).sum().backward()
        return m_.grad

    g32, g64 = ref(torch.float32), ref(torch.float64)
    assert AP.attributed_ok(grad, g32, g64, scale=max(1.0, float(g64.abs().max())))
    if reduce == "sum":                                 # a pure copy of the row gradient: exact
        assert torch.equal(grad.cpu(), gout[c.dst])


# ---------------------------------------------------------------------------------------------------------------------
# ops.gather_combine (EGC): the aggregation with the head / basis combine as its row finish
# ---------------------------------------------------------------------------------------------------------------------
def _combine(agg, coef, K, B, Dh):
    n = agg.shape[0]
    return torch.einsum("nkb,nkbd->nkd", coef.view(n, K, B), agg.view(n, K, B, Dh)).reshape(n, K * Dh)


EGC_SHAPES = [(2, 2, 16), (2, 4, 12), (4, 4, 16), (4, 4, 32), (3, 2, 5), (2, 3, 6), (3, 5, 15), (1, 1, 1)]


@pytest.mark.parametrize("K,B,Dh", EGC_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("reduce", REDUCES)
def test_gather_combine_every_geometry(reduce, K, B, Dh):
    """(K, B, Dh) with M = K*B*Dh at 64 / 96 / 256 / 512 (float4 lane geometries), 30 / 225 / 1 (scalar), Dh = 6 (float4
    aggregate, scalar combine)."""
    from ptgnn_amd import ops
    c = case(1)
    c.assert_hub_plan()
    M = K * B * Dh
    msgs = values(c.E, M, reduce, seed=M + 51)
    coef = torch.randn(c.N, K * B, generator=torch.Generator().manual_seed(M))
    y, cf = msgs.cuda(), coef.cuda()
    mm = reduce in ("max", "min")
    out, agg, arg = ops.gather_combine(y, c.plan, K, B, Dh, reduce, cf, type_bits=0, col=c.plan.perm,
                                       return_agg=True, return_arg=mm)
    inf = ops.gather_combine(y, c.plan, K, B, Dh, reduce, cf, type_bits=0, col=c.plan.perm)
    assert torch.equal(inf.view(I32), out.view(I32)), "the inference form (no aggregate stored) differs"
    agg_c = agg.cpu()
    check_reduce(c, agg_c, msgs, reduce, arg=arg, what=f"egc {reduce} {(K, B, Dh)}")
    plain = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm).cpu()
    assert torch.equal(agg_c[c.small].view(I32), plain[c.small].view(I32)), "agg differs from gather_reduce"
    # the combine of that aggregate: tight against float64 (an in-order fold of B products)
    c64 = _combine(agg_c.double(), coef.double(), K, B, Dh)
    mass = _combine(agg_c.double().abs(), coef.double().abs(), K, B, Dh)
    err = (out.cpu().double() - c64).abs() / (1.0 + mass)
    assert float(err.max()) <= 1e-6, float(err.max())
    # the whole pipeline against float64
    from oracle import scatter_ref
    if mm:
        a32 = AP.first_winner(msgs, c.dst, c.N, reduce)[0]
        a64 = a32.double()
    else:
        a32 = scatter_ref.scatter(msgs, c.dst, dim=0, dim_size=c.N, reduce=reduce)
        a64 = scatter_ref.scatter(msgs.double(), c.dst, dim=0, dim_size=c.N, reduce=reduce)
    assert AP.attributed_ok(out, _combine(a32, coef, K, B, Dh), _combine(a64, coef.double(), K, B, Dh))
    torch.cuda.synchronize()
    assert int(c.plan.hub_tickets(M).abs().sum()) == 0


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_gather_combine_table_form(reduce):
    from ptgnn_amd import ops
    c = case(3)
    c.assert_hub_plan()
    K, B, Dh = 2, 2, 16
    M = K * B * Dh
    y = values(c.N, 3 * M, reduce, seed=61)
    coef = torch.randn(c.N, K * B, generator=torch.Generator().manual_seed(62))
    out, agg, arg = ops.gather_combine(y.cuda(), c.plan, K, B, Dh, reduce, coef.cuda(), return_agg=True,
                                       return_arg=reduce == "max")
    check_reduce(c, agg.cpu(), c.table_msgs(y, M), reduce, arg=arg, what=f"egc table {reduce}")
    c64 = _combine(agg.cpu().double(), coef.double(), K, B, Dh)
    mass = _combine(agg.cpu().double().abs(), coef.double().abs(), K, B, Dh)
    assert float(((out.cpu().double() - c64).abs() / (1.0 + mass)).max()) <= 1e-6


@pytest.mark.parametrize("K,B,Dh,aligned", [(4, 4, 33, True), (3, 3, 29, False), (1, 1, 260, False)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_gather_combine_past_the_fused_row_equals_gather_reduce_and_basis_combine(reduce, K, B, Dh, aligned):
    from ptgnn_amd import ops
    c = case(1)
    M = K * B * Dh
    msgs = values(c.E, M, reduce, seed=M + 71)
    y = msgs.cuda()
    if not aligned:
        y = torch.zeros(c.E, M + 1, device="cuda")[:, 1:]
        y.copy_(msgs.cuda())
    coef = torch.randn(c.N, K * B, generator=torch.Generator().manual_seed(72)).cuda()
    out, agg, arg = ops.gather_combine(y, c.plan, K, B, Dh, reduce, coef, type_bits=0, col=c.plan.perm,
                                       return_agg=True, return_arg=reduce == "max")
    res = ops.gather_reduce(y, c.plan, M, reduce, type_bits=0, col=c.plan.perm, return_arg=reduce == "max")
    a2 = res[0] if isinstance(res, tuple) else res
    assert torch.equal(agg.view(I32), a2.view(I32))
    assert torch.equal(out.view(I32), ops.basis_combine(a2, coef, K, B, Dh).view(I32))
    check_reduce(c, agg.cpu(), msgs, reduce, arg=arg, what="egc past the limit")


# ---------------------------------------------------------------------------------------------------------------------
# PNA: k_pna_rows / k_pna_long_rows, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
PNA_WIDTHS = [1, 3, 5, 63, 64, 65, 68, 130, 256, 257, 300, 516]


@pytest.mark.parametrize("M", PNA_WIDTHS)
def test_pna_forward_and_backward_every_width(M):
    """Edge form with arg (the training path): every lane geometry and column-block count, degrees 255 / 256 / 257 side
    by side and hubs (workgroup-per-row launch), ties on signed zeros at odd widths."""
    from ptgnn_amd import scatter
    c = case(1)
    assert bool((c.deg == AP.K_PNA_LONG).any()) and bool((c.deg == AP.K_PNA_LONG + 1).any())
    msgs = AP.tie_values(c.E, M, seed=M) if M in (5, 65) else values(c.E, M, "sum", seed=M + 81)
    gout = torch.randn(c.N, 15 * M, generator=torch.Generator().manual_seed(M + 82))
    m = msgs.cuda().requires_grad_(True)
    out = scatter.pna_aggregate(m, c.plan, 1.5)
    (out * gout.cuda()).sum().backward()
    with torch.no_grad():
        inf = scatter.pna_aggregate(m.detach(), c.plan, 1.5)          # the inference instantiation (no arg)

    def ref(dtype):
        m_ = msgs.to(dtype).clone().requires_grad_(True)
        o = AP.pna_ref(m_, c.dst, c.N, 1.5)
        (o * gout.to(dtype)).sum().backward()
        return o, m_.grad

    o32, g32 = ref(torch.float32)
    o64, g64 = ref(torch.float64)
    assert AP.attributed_ok(out, o32, o64), "forward"
    assert AP.attributed_ok(inf, o32, o64), "forward without arg"
    assert AP.attributed_ok(m.grad, g32, g64, scale=max(1.0, float(g64.abs().max()))), "backward"


@pytest.mark.parametrize("M", [8, 65, 256])
@pytest.mark.parametrize("dst", [0, 1, 2])
def test_pna_gelu_layernorm_epilogue_on_long_rows(dst, M):
    """The GELU + LayerNorm(15M) finish with no destination term (DST 0, table form T = 3), a per-slot one (DST 1,
    T = 3) and a per-row one (DST 2, T = 1), on rows of every degree including long rows and hubs."""
    from ptgnn_amd import ops
    T = 1 if dst == 2 else 3
    c = case(T)
    assert bool((c.deg > AP.K_PNA_LONG).any())
    g = torch.Generator().manual_seed(M + dst)
    y = torch.randn(c.N, T * M, generator=g)
    yd = torch.randn(c.N, T * M, generator=g) if dst else None
    w, b = torch.rand(15 * M, generator=g) + 0.5, torch.randn(15 * M, generator=g)
    out = ops.pna_aggregate(y.cuda(), c.plan, M, 0.75, ydst=yd.cuda() if dst else None,
                            epilogue=ops.EPI_GELU_LAYERNORM, ln_weight=w.cuda(), ln_bias=b.cuda())

    def ref(dtype):
        o = AP.pna_ref(c.table_msgs(y.to(dtype), M, yd.to(dtype) if dst else None), c.dst, c.N, 0.75)
        return F.layer_norm(F.gelu(o), (15 * M,), w.to(dtype), b.to(dtype), eps=1e-5)

    assert AP.attributed_ok(out, ref(torch.float32), ref(torch.float64))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pna_round_to_half_on_long_rows(dtype):
    from ptgnn_amd import ops, torch_route
    c = case(1)
    assert bool((c.deg > AP.K_PNA_LONG).any())
    M = 16
    m = torch.randn(c.E, M, generator=torch.Generator().manual_seed(91)).to(dtype)
    out = ops.pna_aggregate(m.float().cuda(), c.plan, M, 1.0, type_bits=0, col=c.plan.perm, round_to=dtype).cpu()
    assert torch.equal(out[:, :5 * M], out[:, :5 * M].to(dtype).float())   # block A: message-dtype values
    want = torch_route.pna_aggregate(m, c.dst, c.N, 1)
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    err = (out - want).abs() - ulp * want.abs()
    long = c.deg > AP.K_PNA_LONG
    assert float(err[long].max()) <= 1e-5 * max(1.0, float(want[long].abs().max())), float(err[long].max())
    assert float(err.max()) <= 1e-5 * max(1.0, float(want.abs().max())), float(err.max())


# ---------------------------------------------------------------------------------------------------------------------
# the side-stream and caller-stream hub launches (environment read once per process: a child process)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"PTGNN_AMD_SIDE_MIN_EDGES": "0"},
                                 {"PTGNN_AMD_SIDE_MIN_EDGES": "0", "PTGNN_AMD_HUB_STREAM": "0"}],
                         ids=["side-streams", "caller-stream"])
def test_side_and_caller_stream_hub_paths_in_a_child(env, tmp_path):
    """PTGNN_AMD_SIDE_MIN_EDGES=0: hub chunks and k_long_rows on side streams; with PTGNN_AMD_HUB_STREAM=0 the dedicated
    k_hub_chunks launch on the caller's stream.  The child applies the bars of this module; here its rows of degree
    <= 2048 are compared with the default in-process path, bit for bit."""
    from ptgnn_amd import ops
    _need_gpu()
    dump = tmp_path / "side.pt"
    full = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "agg_paths_side_check.py"), str(dump)], cwd=ROOT,
                       env=full, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + "\n" + r.stderr)[-6000:]
    assert r.returncode == 0, tail
    assert "side-check ok" in r.stdout, tail
    got = torch.load(str(dump))
    import agg_paths_side_check as S
    for name, (T, fn) in S.CASES.items():
        c = case(T)
        mine = fn(c.plan, S.inputs(c.sp, name))
        for k, (a, b) in enumerate(zip(mine, got[name])):
            assert (a is None) == (b is None), (name, k)
            if a is None:
                continue
            a = a.cpu()
            if a.dtype == torch.int32 or name.endswith(("max", "arg")):
                assert torch.equal(a.view(I32), b.view(I32)), (name, k)
            else:
                assert torch.equal(a[c.small].view(I32), b[c.small].view(I32)), (name, k)
    assert ops.HUB_THRESHOLD == AP.HUB_THRESHOLD
