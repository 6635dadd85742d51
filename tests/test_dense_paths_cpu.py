"""The support module of the dense path tests, checked without a GPU: its float64 references against torch's own
float64 Linear / GRUCell and their autograd, its restated dispatches at every threshold from both sides, and the
arithmetic of the constants it copies from the kernels' sources."""
import itertools

import pytest
import torch

import dense_paths as P
from dense_paths import FORCE, GRU_RING, LIN_BN, LIN_RING

REF_TOL = 1e-12


def _close(got, want, tol=REF_TOL):
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    return float((got - want).abs().max()) <= tol * scale if want.numel() else got.shape == want.shape


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [None, "tanh", "relu"])
@pytest.mark.parametrize("bias,addend", [(False, False), (True, False), (True, True)])
def test_linear_reference_equals_torch_float64_linear(act, bias, addend):
    x, w, b = P.linear_case(77, 50, 37, bias=bias)
    add = torch.randn(77, 37) if addend else None
    want = torch.nn.functional.linear(x.double(), w.double(), b.double() if bias else None)
    want = {"tanh": torch.tanh, "relu": torch.relu, None: lambda v: v}[act](want)
    if addend:
        want = want + add.double()
    assert _close(P.linear_ref(x, w, b, act, add), want)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n,m,hd", [(33, 24, 16), (5, 130, 70), (0, 8, 4)])
def test_gru_reference_equals_torch_float64_grucell_and_its_autograd(n, m, hd, bias):
    torch.manual_seed(n + m)
    cell = torch.nn.GRUCell(m, hd, bias=bias).double()
    a = torch.randn(n, m, dtype=torch.float64, requires_grad=True)
    h = torch.randn(n, hd, dtype=torch.float64, requires_grad=True)
    g = torch.randn(n, hd, dtype=torch.float64)
    want = cell(a, h)
    b_ih, b_hh = (cell.bias_ih, cell.bias_hh) if bias else (None, None)
    out, r, z, nn_, gh_n = P.gru_ref(a, h, cell.weight_ih, cell.weight_hh, b_ih, b_hh)
    assert _close(out, want.detach())
    if n == 0:
        return
    # gate-math backward + the four GEMM halves == torch's autograd through the cell
    want.backward(g)
    d_gi, d_gh, d_h = P.gates_backward_ref(g, torch.cat([r, z, nn_, gh_n], 1), h)
    w_ih, w_hh = cell.weight_ih.detach(), cell.weight_hh.detach()
    assert _close(d_gi @ w_ih, a.grad, 1e-11)
    assert _close(d_gh @ w_hh + d_h, h.grad, 1e-11)
    gw_ih, gb_ih = P.weight_grad_ref(a, d_gi)
    gw_hh, gb_hh = P.weight_grad_ref(h, d_gh)
    assert _close(gw_ih, cell.weight_ih.grad, 1e-11) and _close(gw_hh, cell.weight_hh.grad, 1e-11)
    if bias:
        assert _close(gb_ih, cell.bias_ih.grad, 1e-11) and _close(gb_hh, cell.bias_hh.grad, 1e-11)


def test_gates_backward_scale_bounds_the_reference():
    """S is the reference's own formula on absolute values with three factors replaced by upper bounds."""
    a, h, w_ih, w_hh, b_ih, b_hh = P.gru_case(40, 24, 16)
    _, r, z, n, gh_n = P.gru_ref(a, h, w_ih, w_hh, b_ih, b_hh)
    gates = torch.cat([r, z, n, gh_n], 1)
    g = torch.randn(40, 16)
    for ref, s in zip(P.gates_backward_ref(g, gates, h), P.gates_backward_scale(g, gates, h)):
        assert ref.shape == s.shape and bool((ref.abs() <= s * (1 + 1e-9) + 1e-300).all())


@pytest.mark.parametrize("act", [None, "tanh", "relu"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_act_dropout_backward_reference_equals_torch_float64_autograd(act, p):
    torch.manual_seed(3)
    u = torch.randn(257, dtype=torch.float64)
    u[::7] = 0.0                                             # relu at 0: gradient 0
    u.requires_grad_(True)
    keep = (torch.rand(257) >= p) if p > 0 else None
    scale = 1.0 / (1.0 - p)
    y = {"tanh": torch.tanh, "relu": torch.relu, None: lambda v: v}[act](u)
    out = y if keep is None else y * keep.double() * scale
    g = torch.randn(257, dtype=torch.float64)
    (want,) = torch.autograd.grad(out, [u], g)
    got = P.act_dropout_backward_ref(g, y.detach(), keep, scale, act)
    assert _close(got, want, 1e-11)
    if act == "relu":
        assert bool((got[::7] == 0).all())
    assert bool((got.abs() <= P.act_dropout_backward_scale(g, keep, scale) * (1 + 1e-9)).all())


def test_weight_grad_reference_equals_torch_float64_autograd():
    x, w, b = P.linear_case(301, 36, 20)
    lin = torch.nn.Linear(36, 20).double()
    gy = torch.randn(301, 20, dtype=torch.float64)
    lin(x.double()).backward(gy)
    gw, gb = P.weight_grad_ref(x, gy)
    assert _close(gw, lin.weight.grad) and _close(gb, lin.bias.grad)


def test_identity_probe_reads_the_weight_back_exactly():
    w = torch.randn(96, 64)
    x = P.identity_probe(64, 200, offset=70)
    y = (x @ w.t())
    assert torch.equal(y[70:134], w.t()) and float(y[:70].abs().sum()) == 0 and float(y[134:].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_consistent():
    assert P.K_EPI_BYTES == 16 + 8 * P.K_TQ_FLOATS * 4 == 9232
    assert P.resident_lds(256, 128) == P.slab_bytes(256, 128) + P.K_EPI_BYTES
    # the 128-column slab: K = 256 fits, K = 320 does not
    assert 128 * (256 + 4) * 4 + P.K_EPI_BYTES <= 160 * 1024 < 128 * (320 + 4) * 4 + P.K_EPI_BYTES
    # the 64-column slab: K = 576 fits, K = 640 does not
    assert 64 * (576 + 4) * 4 + P.K_EPI_BYTES <= 160 * 1024 < 64 * (640 + 4) * 4 + P.K_EPI_BYTES
    # the GRU's 96-row slab: M + H = 384 fits, 448 does not
    assert P.resident_lds(384, 96) <= P.K_LDS_BUDGET < P.resident_lds(448, 96)
    # both rings fit beside each other twice per CU (two 4-wave workgroups)
    lin_ring = (2 * P.K_LIN_RING_PANEL_FLOATS + P.K_RING_WAVES * P.K_TQ_FLOATS) * 4
    gru_ring = (2 * P.K_RING_PANEL_FLOATS + P.K_RING_WAVES * P.K_TQ_FLOATS) * 4
    assert 2 * lin_ring <= P.K_LDS_BUDGET and 2 * gru_ring <= P.K_LDS_BUDGET
    assert P.RING_MIN_ROWS == 2048 and P.UNITS_PER_CU == 24
    assert [P.blocks_for(w) for w in (32, 64, 96, 128, 160, 384, 36, 100, 132)] == [1, 2, 1, 4, 1, 4, 0, 0, 0]
    # the gate-math backward wraps its grid beyond 65536 * 256 float4 items
    assert P.GATES_BWD_MAX_BLOCKS * 256 == 1 << 24


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_dense_runs_and_the_ragged_row_count(cus):
    for ncs, ring in itertools.product((1, 2, 3, 4, 5), (False, True)):
        rows = P.ragged_run_rows(cus, ncs, ring)
        nrb = (rows + 31) // 32
        rps, run_len = P.dense_runs(nrb, ncs, 2 * cus if ring else cus)
        assert run_len > 1 and nrb % run_len != 0 and rows % 32 != 0
        assert (rps - 1) * run_len < nrb <= rps * run_len            # no empty run, every unit covered


# ---------------------------------------------------------------------------------------------------------------------
# dispatch restatements
# ---------------------------------------------------------------------------------------------------------------------
F = {FORCE: "1"}


def test_linear_route_thresholds_from_both_sides():
    name = lambda *a, **k: P.linear_route(*a, **k).name
    big = 1 << 20
    # 128-column slab: K = 256 resident, K = 320 takes 64-column slabs
    assert name(big, 256, 128) == "resident_nb4" and name(big, 320, 128) == "resident_bn64"
    # 64-column slab: K = 576 resident, K = 640 the ring
    assert name(big, 576, 256) == "resident_bn64" and name(big, 640, 256) == "ring"
    # bn-64 needs n_out % 128 == 0 and n_out <= 256
    assert name(big, 320, 384) == "ring" and name(big, 320, 160, env=F) == "tile_nj2"
    # four column slabs at most (unless the floors are lifted)
    assert P.linear_route(big, 64, 512) == P.Route("resident_nb4", 1, 4)
    assert name(big, 64, 544) == "tile_nj2" and P.linear_route(big, 64, 544, env=F) == P.Route("resident_nb4", 1, 5)
    # ring floor
    assert name(2047, 768, 128) == "tile_nj1" and name(2048, 768, 128) == "ring"
    assert name(1, 768, 128, env=F) == "ring"
    assert name(big, 768, 128, env={LIN_RING: "0"}) == "tile_nj1"        # nothing fits, the ring is off
    # unit floor for cus as a parameter
    for cus in (256, 304, 8):
        at = cus * P.UNITS_PER_CU
        assert name(32 * (at - 1), 128, 128, cus=cus) == "tile_nj1"
        assert name(32 * (at - 1) + 1, 128, 128, cus=cus) == "resident_nb4"
        assert name(32 * at // 2 - 32, 64, 256, cus=cus) == "tile_nj2"   # two slabs: half the rows
        assert name(32 * at // 2 - 31, 64, 256, cus=cus) == "resident_nb4"
    # switches
    assert name(64, 128, 128, env={FORCE: "1", LIN_RING: "1"}) == "ring"
    assert name(64, 128, 128, env={FORCE: "1", LIN_BN: "64"}) == "resident_bn64"
    assert name(big, 320, 128, env={LIN_BN: "128"}) == "ring"
    assert name(big, 128, 128, mode=0) == "tile_nj1" and name(big, 128, 256, mode=0) == "tile_nj2"
    # shapes of the tile kernel only
    for kw in (dict(k=130), dict(n_out=129), dict(n_out=130), dict(ld_x=129), dict(aligned=False)):
        args = dict(rows=big, k=128, n_out=128, env=F)
        args.update(kw)
        assert P.linear_route(**args).name.startswith("tile_nj")
    # stores
    assert P.linear_route(big, 128, 128, ld_y=132).vec_store == 1
    assert P.linear_route(big, 128, 128, ld_y=131).vec_store == 0
    assert P.linear_route(big, 128, 128, ld_y=132, y_aligned=False).vec_store == 0
    # the add epilogue lives in the dwordx4 stores of the streaming kernels
    assert name(big, 128, 128, addend=True) == "resident_nb4"
    assert name(big, 128, 128, addend=True, ld_y=131) == "unsupported"
    assert name(big, 128, 128, addend=True, ld_add=130) == "unsupported"
    assert name(100, 128, 128, addend=True) == "unsupported" and name(big, 100, 128, addend=True) == "unsupported"
    assert name(0, 128, 128) is None


def test_gru_route_thresholds_from_both_sides():
    assert P.gru_route(1, 128, 256) == "gru_resident" and P.gru_route(1, 192, 256) == "gru_ring"   # M + H 384 | 448
    assert P.gru_route(1, 192, 256, env={GRU_RING: "0"}) == "gru_tile_aligned"
    assert P.gru_route(1, 64, 64, env={GRU_RING: "1"}) == "gru_ring"
    assert P.gru_route(1, 64, 64, mode=0) == "gru_tile_aligned"
    assert P.gru_route(5, 24, 16) == "gru_tile_aligned" and P.gru_route(5, 130, 70) == "gru_tile_unaligned"
    assert P.gru_route(5, 64, 64, ld_out=128) == "gru_resident" and P.gru_route(5, 64, 64, ld_out=67) == "gru_tile_aligned"
    assert P.gru_route(5, 64, 64, ld_a=65) == "gru_tile_unaligned"
    assert P.gru_route(0, 64, 64) is None


def test_wgrad_route_covers_every_block_pair():
    seen = {P.wgrad_route(10, k, n) for k in P.WGRAD_STREAM_WIDTHS for n in P.WGRAD_STREAM_WIDTHS}
    assert seen == set(P.WGRAD_ROUTES) - {"wgrad_tile"}
    assert P.wgrad_route(10, 64, 32) == "wgrad_stream_1x2"               # side A = n_out, side B = k
    for w in P.WGRAD_TILE_WIDTHS:
        assert P.wgrad_route(10, w, 64) == "wgrad_tile" and P.wgrad_route(10, 64, w) == "wgrad_tile"
    assert P.wgrad_route(10, 37, 64) == "unsupported" and P.wgrad_route(0, 64, 64) is None
    # small inputs: one workgroup takes 256 rows on either kernel, so 256 | 257 rows is a workgroup / chunk boundary
    for cus in (256, 304):
        for k, n in ((64, 64), (384, 160), (36, 100), (132, 132)):
            assert P.wgrad_rows_per_workgroup(257, k, n, cus) == 256


def test_case_matrix_reaches_every_route_name():
    seen = set()
    for cus in (256, 304):
        for k, n_out, env, mode in P.LINEAR_SHAPES:
            ncs_guess = max(1, (n_out + 127) // 128)
            for rows in P.row_counts(cus, ncs_guess):
                seen.add(P.linear_route(rows, k, n_out, env=env, cus=cus, mode=mode).name)
        for m, hd in P.GRU_SHAPES:
            for env in ({}, {GRU_RING: "1"}):
                seen.add(P.gru_route(33, m, hd, env=env))
        for k in P.WGRAD_STREAM_WIDTHS + P.WGRAD_TILE_WIDTHS:
            for n in P.WGRAD_STREAM_WIDTHS + P.WGRAD_TILE_WIDTHS:
                seen.add(P.wgrad_route(33, k, n))
        assert seen == set(P.ALL_ROUTES)
    assert {P.counter_of(r) for r in P.ALL_ROUTES} == set(P.DENSE_COUNTERS)
    # the matrix holds the widths and depths the kernels' column / K guards depend on
    assert {n for _, n, _, _ in P.LINEAR_SHAPES} >= {32, 64, 96, 128, 160, 224, 256, 288, 384, 512, 544, 129, 130}
    assert {k for k, _, _, _ in P.LINEAR_SHAPES} >= {64, 128, 256, 320, 576, 640, 768}
