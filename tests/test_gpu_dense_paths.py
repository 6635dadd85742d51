"""Every dense dispatch route -- Linear, fused GRU cell, weight gradient, and the two element-wise backward kernels --
against float64, at the row tails, widths and depths where the kernels switch paths (tests/dense_paths.py).

Every case first predicts its route with the plain-Python restatement of the host dispatch and then asserts it from the
library's launch counters: a prediction the counters do not confirm is a failure.  `SEEN` collects the asserted route
names; the last test of the file asserts the set is complete (and runs a small witness of any route a partial
selection of this file left out).

Tolerances: forward 1e-5 * max(1, |want|inf), gradients 2e-5 * max(1, |want|inf) (the project's bars); the element-wise
backward kernels have derived bounds (k roundings of bounded factors: k * 2^-24 * S with headroom, see the tests).

The 200 001-row weight gradient is the one bound not known in advance: plain fp32 `torch` CPU `gy.t() @ x` was measured
against float64 on this file's inputs (reference arithmetic, not the code under test) and the test allows
max(2e-5 * max(1, |want|inf), 4 * that error).  The fp32 error depends on how the host BLAS blocks the 200 001-term
sums, so the test recomputes it on every run and prints it beside the kernel's own error; on the MI355X host:

    (k, n_out)    |want|inf   fp32 torch error   4 x error   project bound   bound used   kernel error
    (64, 64)        1.70e3        2.1e-3           8.3e-3        3.4e-2        3.4e-2        4.9e-4
    (128, 384)      1.79e3        2.3e-3           9.0e-3        3.6e-2        3.6e-2        7.9e-4
    (36, 100)       1.68e3        1.7e-2           7.0e-2        3.4e-2        7.0e-2        6.6e-4
"""
import contextlib
import copy

import pytest
import torch

import dense_paths as P
from dense_paths import FORCE, GRU_RING, LIN_RING, TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

ACTS = (None, "tanh", "relu")
SEEN = set()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_env(monkeypatch, env):
    for name in P.ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


@contextlib.contextmanager
def _mode(mode):
    from ptgnn_amd import ops
    prev = ops.set_gemm_mode(mode)
    try:
        yield
    finally:
        ops.set_gemm_mode(prev)


def _counted(fn, expect, what=""):
    """Run fn; the dense launch counters must have moved by exactly `expect` ({counter: launches})."""
    from ptgnn_amd import ops
    before = ops.launch_counts()
    out = fn()
    since = {k: v for k, v in ops.launches_since(before).items() if k in P.DENSE_COUNTERS}
    assert since == expect, f"{what}: predicted launches {expect}, the library counted {since}"
    return out


def _routed(fn, name, what=""):
    out = _counted(fn, {P.counter_of(name): 1} if name else {}, f"{what} route {name}")
    if name:
        SEEN.add(name)
    return out


def _assert_close(got, want64, tol, what, bn=None):
    """|got - want64| <= tol * max(1, |want64|inf); on a miss name the first wrong (row, column) and its slab."""
    want64 = want64.to(got.device)
    assert got.shape == want64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want64.shape)}"
    if got.numel() == 0:
        return
    bound = tol * max(1.0, float(want64.abs().max()))
    err = (got.double() - want64).abs()
    bad = ~(err <= bound)                      # NaN counts as wrong
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        slab = f", slab {idx[-1] // bn}" if bn else ""
        raise AssertionError(f"{what}: {int(bad.sum())} wrong, first at {idx}{slab}: got {got[tuple(idx)].item()!r} "
                             f"want {want64[tuple(idx)].item()!r} (max err {float(err.nan_to_num(nan=float('inf')).max()):.3e}, "
                             f"bound {bound:.3e})")


def _assert_bounded(got, want64, scale64, k, what):
    """Derived bound of an element-wise kernel: |got - want| <= k * 2^-24 * S element-wise."""
    err = (got.double() - want64.to(got.device)).abs()
    bound = k * P.EPS32 * scale64.to(got.device)
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} beyond {k} roundings, first at {idx}: got {got[idx].item()!r} "
                             f"want {want64[idx].item()!r} bound {bound[idx].item():.3e}")


def _act64(v, act):
    return torch.tanh(v) if act == "tanh" else (torch.relu(v) if act == "relu" else v)


def _bn_of(route, n_out):
    return 64 if route.name == "resident_bn64" else min(n_out, 128)


def _same_bits(a, b, act, what):
    """The project's claim: one K order on every Linear kernel -- equal bits without an activation and under relu; the
    tile kernel's tanh is libm's, the streaming kernels' the hardware exponential: within 1e-6."""
    if act == "tanh":
        assert float((a - b).abs().max()) <= 1e-6, f"{what}: tanh results differ by more than 1e-6"
    else:
        if not torch.equal(a, b):
            idx = torch.nonzero(a != b)[0].tolist()
            raise AssertionError(f"{what}: bits differ, first at {idx}: {a[tuple(idx)].item()!r} != {b[tuple(idx)].item()!r}")


# ---------------------------------------------------------------------------------------------------------------------
# Linear forward
# ---------------------------------------------------------------------------------------------------------------------
def _shape_id(v):
    k, n_out, env, mode = v
    sw = "".join(f"-{key.replace('PTGNN_AMD_', '').lower()}{val}" for key, val in sorted(env.items()))
    return f"k{k}-n{n_out}{sw}-{'tile' if mode == 0 else 'stream'}"


def _linear_rows(k, n_out, env, mode, cus):
    probe = P.linear_route(4096, k, n_out, env=env, cus=cus, mode=mode)
    return P.row_counts(cus, max(probe.slabs, 1) if not probe.name.startswith("tile") else 1, probe.name == "ring")


@pytest.mark.parametrize("shape", P.LINEAR_SHAPES, ids=_shape_id)
def test_linear_every_route_matches_float64_and_the_other_kernels(shape, monkeypatch):
    from ptgnn_amd import ops
    k, n_out, env, mode = shape
    cus = _cus()
    for rows in _linear_rows(k, n_out, env, mode, cus):
        x, w, b = P.linear_case(rows, k, n_out)
        raw = (x.double() @ w.double().t()).cuda()
        xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
        route = P.linear_route(rows, k, n_out, env=env, cus=cus, mode=mode)
        both_resident_and_ring = route.name.startswith("resident") and n_out % 128 == 0
        for bias in (None, bc):
            for act in ACTS:
                what = f"linear rows={rows} k={k} n_out={n_out} bias={bias is not None} act={act} route={route.name}"
                want = _act64(raw if bias is None else raw + bias.double(), act)
                _set_env(monkeypatch, env)
                with _mode(mode):
                    got = _routed(lambda: ops.linear(xc, wc, bias, act=act), route.name, what)
                _assert_close(got, want, TOL, what, _bn_of(route, n_out))
                if not route.name.startswith("tile"):
                    with _mode("tile"):
                        tile = _counted(lambda: ops.linear(xc, wc, bias, act=act), {"k_linear_tlp": 1}, what + " (tile)")
                    _same_bits(got, tile, act, what + " vs tile kernel")
                if both_resident_and_ring:
                    _set_env(monkeypatch, {FORCE: "1", LIN_RING: "1"})
                    ring = _routed(lambda: ops.linear(xc, wc, bias, act=act), "ring", what + " (forced ring)")
                    _same_bits(got, ring, act, what + " vs ring")


@pytest.mark.parametrize("shape", P.LINEAR_SHAPES, ids=_shape_id)
def test_linear_identity_probe_reads_the_weight_back_bit_for_bit(shape, monkeypatch):
    """x = I_K at row 37 between zero rows, no bias: y[37 : 37 + K] == W^T exactly and every other row is exactly zero,
    whatever the route -- a mis-indexed K chunk, column block or row fails exactly."""
    from ptgnn_amd import ops
    k, n_out, env, mode = shape
    cus = _cus()
    rows, off = k + 37 + 45, 37
    w = P.linear_case(rows, k, n_out)[1]
    xc, wc = P.identity_probe(k, rows, off).cuda(), w.cuda()
    route = P.linear_route(rows, k, n_out, env=env, cus=cus, mode=mode)
    for act in (None, "relu"):
        _set_env(monkeypatch, env)
        with _mode(mode):
            y = _routed(lambda: ops.linear(xc, wc, None, act=act), route.name, f"identity probe {_shape_id(shape)}")
        want = wc.t() if act is None else torch.relu(wc.t())
        band = y[off:off + k]
        if not torch.equal(band, want):
            idx = torch.nonzero(band != want)[0].tolist()
            raise AssertionError(f"identity probe {_shape_id(shape)} route {route.name} act={act}: y[{off + idx[0]}, {idx[1]}] = "
                                 f"{band[tuple(idx)].item()!r}, W[{idx[1]}, {idx[0]}] = {want[tuple(idx)].item()!r} "
                                 f"(slab {idx[1] // _bn_of(route, n_out)})")
        assert float(y[:off].abs().sum()) == 0.0 and float(y[off + k:].abs().sum()) == 0.0


def test_linear_tile_only_layouts_match_float64(monkeypatch):
    """ld_x % 4 != 0 and a base pointer off 16 bytes send a streaming shape to the tile kernel's unaligned staging."""
    from ptgnn_amd import ops
    _set_env(monkeypatch, {FORCE: "1"})
    cus = _cus()
    for rows in (1, 33, 129, 2049):
        x, w, b = P.linear_case(rows, 128, 128)
        want = P.linear_ref(x, w, b, "tanh")
        wide = torch.zeros(rows, 131, device="cuda")                    # ld_x = 131
        wide[:, :128] = x.cuda()
        route = P.linear_route(rows, 128, 128, ld_x=131, env={FORCE: "1"}, cus=cus)
        assert route.name == "tile_nj1"
        got = _routed(lambda: ops.linear(wide[:, :128], w.cuda(), b.cuda(), act="tanh"), route.name, "ld_x 131")
        _assert_close(got, want, TOL, f"ld_x % 4 != 0 rows={rows}")
        flat = torch.zeros(rows * 128 + 1, device="cuda")               # storage offset 1: base pointer off 16 bytes
        xo = flat[1:].view(rows, 128)
        xo.copy_(x)
        assert xo.data_ptr() % 16 != 0
        route = P.linear_route(rows, 128, 128, aligned=False, env={FORCE: "1"}, cus=cus)
        got = _routed(lambda: ops.linear(xo, w.cuda(), b.cuda(), act="tanh"), route.name, "offset base")
        _assert_close(got, want, TOL, f"unaligned base rows={rows}")


def test_linear_real_size_thresholds(monkeypatch):
    """Without PTGNN_AMD_FORCE_STREAM: the unit floor CUs * 24, the ring's 2048-row floor and the 4-slab limit."""
    from ptgnn_amd import ops
    _set_env(monkeypatch, {})
    cus = _cus()
    at = cus * P.UNITS_PER_CU
    cases = [(32 * (at - 1), 128, 128, "tile_nj1"), (32 * (at - 1) + 1, 128, 128, "resident_nb4"),
             (2047, 768, 128, "tile_nj1"), (2048, 768, 128, "ring"),
             (32 * (at // 4), 64, 512, "resident_nb4"), (32 * (at // 4), 64, 544, "tile_nj2")]
    for rows, k, n_out, expect in cases:
        route = P.linear_route(rows, k, n_out, cus=cus)
        assert route.name == expect, (rows, k, n_out, route)
        x, w, b = P.linear_case(rows, k, n_out)
        what = f"threshold rows={rows} k={k} n_out={n_out} route={route.name}"
        got = _routed(lambda: ops.linear(x.cuda(), w.cuda(), b.cuda(), act="relu"), route.name, what)
        _assert_close(got, P.linear_ref(x, w, b, "relu"), TOL, what, _bn_of(route, n_out))


# ---------------------------------------------------------------------------------------------------------------------
# strided views with sentinels
# ---------------------------------------------------------------------------------------------------------------------
VIEW_SHAPES = ((256, 128, {FORCE: "1"}, 1), (576, 256, {FORCE: "1"}, 1), (768, 128, {FORCE: "1"}, 1), (128, 160, {FORCE: "1"}, 1),
               (128, 96, {}, 0), (100, 72, {FORCE: "1"}, 1))


@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=_shape_id)
def test_linear_strided_views_leave_their_surroundings_untouched(shape, monkeypatch):
    from ptgnn_amd import ops
    k, n_out, env, mode = shape
    cus = _cus()
    for rows in (1, 33, 127, 2049):
        x, w, b = P.linear_case(rows, k, n_out)
        want = P.linear_ref(x, w, b, "tanh")
        xbuf = torch.full((rows, k + 8), float("nan"), device="cuda")
        xbuf[:, 4:4 + k] = x.cuda()
        xv = xbuf[:, 4:4 + k]                                        # column slice, rows still 16-byte aligned
        _set_env(monkeypatch, env)
        with _mode(mode):
            flat = ops.linear(x.cuda(), w.cuda(), b.cuda(), act="tanh")
        for pad, col0 in ((8, 4), (7, 3)):                           # ld_y % 4 == 0 | ld_y % 4 != 0: dword stores
            buf = torch.full((rows + 3, n_out + pad), float("nan"), device="cuda")
            out = buf[:rows, col0:col0 + n_out]
            route = P.linear_route(rows, k, n_out, ld_x=k + 8, ld_y=n_out + pad, y_aligned=(col0 % 4 == 0), env=env,
                                   cus=cus, mode=mode)
            assert route.vec_store == (1 if pad == 8 else 0)
            what = f"strided view rows={rows} {_shape_id(shape)} ld_y={n_out + pad} route={route.name}"
            with _mode(mode):
                _routed(lambda: ops.linear(xv, w.cuda(), b.cuda(), act="tanh", out=out), route.name, what)
            _assert_close(out, want, TOL, what, _bn_of(route, n_out))
            assert torch.equal(out, flat), what + ": differs from the contiguous call"
            inside = torch.zeros_like(buf, dtype=torch.bool)
            inside[:rows, col0:col0 + n_out] = True
            assert bool(buf[~inside].isnan().all()), what + ": a sentinel outside the view was overwritten"


GRU_VIEW_CASES = ((24, 16, {}), (64, 64, {}), (64, 64, {GRU_RING: "1"}), (256, 256, {}))


@pytest.mark.parametrize("m,hd,env", GRU_VIEW_CASES)
def test_gru_out_view_and_gates_write_nothing_past_the_last_row(m, hd, env, monkeypatch):
    """`out=` as the right half of a concat-residual buffer (ld_out = 2 hd) and an over-allocated gates buffer: the
    streaming kernels store through descriptors that end at the last valid row."""
    from ptgnn_amd import _lib, ops
    lib = _lib.load()
    for n in (1, 31, 33, 129, 2049):
        a, h, w_ih, w_hh, b_ih, b_hh = P.gru_case(n, m, hd)
        want = P.gru_ref(a, h, w_ih, w_hh, b_ih, b_hh)
        args = [t.cuda() for t in (a, h, w_ih, w_hh, b_ih, b_hh)]
        _set_env(monkeypatch, env)
        route = P.gru_route(n, m, hd, ld_out=2 * hd, env=env)
        buf = torch.full((n + 2, 2 * hd), float("nan"), device="cuda")
        out = buf[:n, hd:]
        what = f"gru out view n={n} m={m} hd={hd} route={route}"
        _routed(lambda: ops.gru_cell(*args, out=out), route, what)
        _assert_close(out, want[0], TOL, what)
        assert bool(buf[:, :hd].isnan().all()) and bool(buf[n:].isnan().all()), what + ": sentinel overwritten"
        assert torch.equal(out, ops.gru_cell(*args)), what + ": differs from the contiguous call"
        # training form through the C ABI: caller-owned, over-allocated gates
        gates = torch.full((n + 2, 4 * hd), float("nan"), device="cuda")
        out2 = torch.full((n + 2, hd), float("nan"), device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        route = P.gru_route(n, m, hd, env=env)

        def train():
            _lib.check(lib.ptgnn_amd_gru_cell_train_f32(args[0].data_ptr(), m, args[1].data_ptr(), hd, args[2].data_ptr(),
                                                        args[3].data_ptr(), args[4].data_ptr(), args[5].data_ptr(), n, m,
                                                        hd, out2.data_ptr(), hd, gates.data_ptr(), st), "gru_cell_train")
        _routed(train, route, what + " (gates)")
        assert bool(gates[n:].isnan().all()) and bool(out2[n:].isnan().all()), what + ": write past row n - 1"
        _assert_close(gates[:n], torch.cat(want[1:], 1), TOL, what + " gates")
        assert torch.equal(out2[:n], out)


# ---------------------------------------------------------------------------------------------------------------------
# linear_add
# ---------------------------------------------------------------------------------------------------------------------
ADD_SHAPES = ((64, 32), (128, 64), (256, 96), (256, 128), (128, 160), (576, 256), (768, 128), (64, 544))


@pytest.mark.parametrize("k,n_out", ADD_SHAPES)
def test_linear_add_matches_float64_on_every_streaming_route(k, n_out, monkeypatch):
    from ptgnn_amd import ops
    env = {FORCE: "1"}
    cus = _cus()
    for rows in (1, 33, 129, 2049):
        x, w, b = P.linear_case(rows, k, n_out)
        addbuf = torch.randn(rows, n_out + 8, generator=torch.Generator().manual_seed(rows))
        add = addbuf[:, 4:4 + n_out]                                  # strided addend, rows 16-byte aligned
        addc = addbuf.cuda()[:, 4:4 + n_out]
        route = P.linear_route(rows, k, n_out, addend=True, ld_add=n_out + 8, env=env, cus=cus)
        assert route.name not in ("unsupported", None) and not route.name.startswith("tile")
        for bias, act in ((None, None), (b, "tanh"), (b, "relu")):
            what = f"linear_add rows={rows} k={k} n_out={n_out} act={act} route={route.name}"
            _set_env(monkeypatch, env)
            got = _routed(lambda: ops.linear_add(x.cuda(), w.cuda(), addc, bias.cuda() if bias is not None else None, act=act),
                          route.name, what)
            _assert_close(got, P.linear_ref(x, w, bias, act, add), TOL, what, _bn_of(route, n_out))


@pytest.mark.parametrize("rows,k,n_out,ld_add,mode", [(300, 100, 128, None, 1), (300, 128, 130, None, 1), (300, 128, 128, 131, 1),
                                                      (300, 128, 128, None, 0), (1, 50, 37, None, 1)])
def test_linear_add_unsupported_shapes_fall_back_to_the_same_sum(rows, k, n_out, ld_add, mode, monkeypatch):
    from ptgnn_amd import ops
    env = {FORCE: "1"}
    cus = _cus()
    x, w, b = P.linear_case(rows, k, n_out)
    addbuf = torch.randn(rows, ld_add or n_out, generator=torch.Generator().manual_seed(5))
    add, addc = addbuf[:, :n_out], addbuf.cuda()[:, :n_out]
    assert P.linear_route(rows, k, n_out, addend=True, ld_add=ld_add, env=env, cus=cus, mode=mode).name == "unsupported"
    plain = P.linear_route(rows, k, n_out, env=env, cus=cus, mode=mode)        # what the host runs instead
    _set_env(monkeypatch, env)
    with _mode(mode):
        got = _routed(lambda: ops.linear_add(x.cuda(), w.cuda(), addc, b.cuda(), act="tanh"), plain.name, "linear_add fall-back")
    _assert_close(got, P.linear_ref(x, w, b, "tanh", add), TOL, f"linear_add fall-back {rows}x{k}->{n_out}")


# ---------------------------------------------------------------------------------------------------------------------
# GRU forward with gates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,hd", P.GRU_SHAPES)
def test_gru_every_route_matches_float64_with_gates(m, hd, monkeypatch):
    from ptgnn_amd import ops
    cus = _cus()
    for n in (0,) + P.row_counts(cus, hd // 32 if hd % 32 == 0 else 1):
        a, h, w_ih, w_hh, b_ih, b_hh = P.gru_case(n, m, hd)
        want = P.gru_ref(a, h, w_ih, w_hh, b_ih, b_hh)
        args = [t.cuda() for t in (a, h, w_ih, w_hh, b_ih, b_hh)]
        _set_env(monkeypatch, {})
        route = P.gru_route(n, m, hd)
        what = f"gru n={n} m={m} hd={hd} route={route}"
        out = _routed(lambda: ops.gru_cell(*args), route, what)
        out_t, gates = _routed(lambda: ops.gru_cell_train(*args), route, what + " (train)")
        assert torch.equal(out, out_t), what + ": gru_cell and gru_cell_train differ"
        _assert_close(out, want[0], TOL, what)
        _assert_close(gates, torch.cat(want[1:], 1), TOL, what + " gates r|z|n|gh_n")
        if route == "gru_resident":
            _set_env(monkeypatch, {GRU_RING: "1"})
            ring, ring_gates = _routed(lambda: ops.gru_cell_train(*args), "gru_ring", what + " (forced ring)")
            assert torch.equal(ring, out) and torch.equal(ring_gates, gates), what + ": ring and resident bits differ"
        if route in ("gru_resident", "gru_ring"):
            with _mode("tile"):
                tile = _routed(lambda: ops.gru_cell(*args), "gru_tile_aligned", what + " (tile)")
            assert float((tile - out).abs().max()) <= 1e-6, what + ": tile kernel differs by more than 1e-6"


# ---------------------------------------------------------------------------------------------------------------------
# element-wise backward kernels
# ---------------------------------------------------------------------------------------------------------------------
def _gates_case(n, hd, m=8):
    from ptgnn_amd import ops
    a, h, w_ih, w_hh, b_ih, b_hh = (t.cuda() for t in P.gru_case(n, m, hd))
    _, gates = ops.gru_cell_train(a, h, w_ih, w_hh, b_ih, b_hh)
    g = torch.randn(n, hd, generator=torch.Generator().manual_seed(n + hd)).cuda()
    return g, gates, h


def _check_gates_backward(got, g, gates, h, what, device="cpu"):
    want = P.gates_backward_ref(g, gates, h, device)
    scale = P.gates_backward_scale(g, gates, h, device)
    for name, o, w_, s in zip(("d_gi", "d_gh", "d_h"), got, want, scale):
        _assert_bounded(o, w_, s, 8, f"{what} {name}")


@pytest.mark.parametrize("hd", [4, 36, 128])
@pytest.mark.parametrize("n", [1, 33, 1000])
def test_gru_gates_backward_matches_float64_autograd(n, hd):
    """Every output is at most 6 fp32 roundings of bounded factors: |got - want64| <= 8 * 2^-24 * S element-wise."""
    from ptgnn_amd import ops
    g, gates, h = _gates_case(n, hd)
    got = ops.gru_gates_backward(g, gates, h)
    _check_gates_backward(got, g, gates, h, f"gates backward n={n} hd={hd}")
    # strided grad_out and h: column slices of wider buffers
    gbuf = torch.full((n, hd + 8), float("nan"), device="cuda")
    hbuf = torch.full((n, 2 * hd), float("nan"), device="cuda")
    gbuf[:, 4:4 + hd], hbuf[:, hd:] = g, h
    strided = ops.gru_gates_backward(gbuf[:, 4:4 + hd], gates, hbuf[:, hd:])
    for o, s in zip(got, strided):
        assert torch.equal(o, s), f"gates backward n={n} hd={hd}: strided inputs change the result"


def test_gru_gates_backward_grid_stride_wrap():
    """n * hd / 4 just above 65536 * 256 items: the capped grid wraps once, the wrapped rows are the last ones."""
    from ptgnn_amd import ops
    n, hd = 263168, 256
    assert n * hd // 4 > P.GATES_BWD_MAX_BLOCKS * 256 and (n - 2048) * hd // 4 < P.GATES_BWD_MAX_BLOCKS * 256
    g, gates, h = _gates_case(n, hd, m=64)
    got = ops.gru_gates_backward(g, gates, h)
    for lo in range(0, n, 32896):                                        # float64 autograd on the device, by row ranges
        hi = min(n, lo + 32896)
        _check_gates_backward([o[lo:hi] for o in got], g[lo:hi], gates[lo:hi], h[lo:hi],
                              f"gates backward wrap rows {lo}:{hi}", device="cuda")


def test_gru_gates_backward_refuses_widths_off_four():
    from ptgnn_amd import _lib, ops
    n, hd = 5, 6
    g, h = torch.randn(n, hd, device="cuda"), torch.randn(n, hd, device="cuda")
    gates = torch.rand(n, 4 * hd, device="cuda")
    with pytest.raises(_lib.PtgnnAmdError, match=f"code {_lib.EUNSUPPORTED}"):
        ops.gru_gates_backward(g, gates, h)


@pytest.mark.parametrize("count", [1, 3, 255, 256, 257, 1000003])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("masked", [False, True])
def test_act_dropout_backward_matches_float64_autograd(count, act, masked):
    """grad * (keep ? scale : 0) * act'(y) with S = |grad| * scale and (1 - y^2) -> 1.  Relative to S the fp32 scale
    and grad * scale err by 2^-24 each, y^2 by 2^-24 y^2, 1 - y^2 by 2^-24 (1 - y^2) and the last product by 2^-24:
    |got - want64| <= 4 * 2^-24 * S.  Without a mask the kernel's multiplier is 1 and `scale` is not read."""
    from ptgnn_amd import ops
    gen = torch.Generator().manual_seed(count)
    u = torch.randn(1, count, generator=gen)
    u[:, ::5] = 0.0                                                      # relu: y == 0 has gradient 0
    y = _act64(u, act).float()
    g = torch.randn(1, count, generator=gen)
    keep = (torch.rand(1, count, generator=gen) >= 0.3) if masked else None
    scale = 1.0 / (1.0 - 0.3) if masked else 1.7                         # scale != 1 either way
    got = ops.act_dropout_backward(g.cuda(), y.cuda(), keep.cuda() if masked else None, scale, act)
    want = P.act_dropout_backward_ref(g, y, keep, scale, act)
    s = P.act_dropout_backward_scale(g, keep, scale)
    _assert_bounded(got, want, s, 4, f"act_dropout_backward count={count} act={act} masked={masked}")
    if act == "relu":
        assert float(got[:, ::5].abs().sum()) == 0.0
    assert got.shape == g.shape


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_check(rows, k, n_out, strided=False, tol_floor=None):
    from ptgnn_amd import ops
    gen = torch.Generator().manual_seed(rows + 31 * k + n_out)
    x, gy = torch.randn(rows, k, generator=gen), torch.randn(rows, n_out, generator=gen)
    want_w, want_b = P.weight_grad_ref(x, gy)
    xc, gc = x.cuda(), gy.cuda()
    if strided:
        xb = torch.full((rows, k + 8), float("nan"), device="cuda")
        gb = torch.full((rows, 2 * n_out + 4), float("nan"), device="cuda")
        xb[:, 4:4 + k], gb[:, n_out + 4:] = xc, gc
        xc, gc = xb[:, 4:4 + k], gb[:, n_out + 4:]
    route = P.wgrad_route(rows, k, n_out)
    what = f"weight grad rows={rows} k={k} n_out={n_out} strided={strided} route={route}"
    gw, gb_ = _routed(lambda: ops.linear_weight_grad(xc, gc, want_bias=True), route, what)
    alone = _routed(lambda: ops.linear_weight_grad(xc, gc), route, what + " (no bias)")
    again, again_b = ops.linear_weight_grad(xc, gc, want_bias=True)
    assert torch.equal(gw, alone), what + ": the bias output changes grad_w"
    assert torch.equal(gw, again) and torch.equal(gb_, again_b), what + ": two calls differ"
    tol = GRAD_TOL
    if tol_floor is not None:      # 4 x the error of plain fp32 torch on the same inputs, if that is the larger
        ref32 = float(((gy.t() @ x).double() - want_w).abs().max())
        scale = max(1.0, float(want_w.abs().max()))
        print(f"{what}: |want|inf {scale:.3e} fp32 torch error {ref32:.3e} bound {max(GRAD_TOL * scale, 4 * ref32):.3e} "
              f"kernel error {float((gw.cpu().double() - want_w).abs().max()):.3e}")
        tol = max(GRAD_TOL, 4.0 * ref32 / scale)
    _assert_close(gw, want_w, tol, what)
    _assert_close(gb_, want_b, GRAD_TOL, what + " bias")


@pytest.mark.parametrize("k", P.WGRAD_STREAM_WIDTHS)
@pytest.mark.parametrize("n_out", P.WGRAD_STREAM_WIDTHS)
def test_weight_grad_streaming_block_pairs_match_float64(k, n_out):
    cus = _cus()
    assert P.wgrad_rows_per_workgroup(257, k, n_out, cus) == 256       # 256 | 257: one workgroup | two
    for rows in (1, 31, 33, 255, 256, 257):
        _wgrad_check(rows, k, n_out)
    _wgrad_check(1000, k, n_out, strided=True)


@pytest.mark.parametrize("k,n_out", [(36, 100), (100, 36), (132, 132), (36, 64), (128, 100)])
def test_weight_grad_tile_widths_match_float64(k, n_out):
    cus = _cus()
    assert P.wgrad_rows_per_workgroup(257, k, n_out, cus) == 256       # 256 | 257: one chunk | two
    for rows in (1, 31, 33, 255, 256, 257):
        _wgrad_check(rows, k, n_out)
    _wgrad_check(1000, k, n_out, strided=True)


@pytest.mark.parametrize("k,n_out", [(64, 64), (128, 384), (36, 100)])
def test_weight_grad_of_200001_rows(k, n_out):
    _wgrad_check(200001, k, n_out, tol_floor=True)


def test_weight_grad_zero_rows_launches_nothing():
    from ptgnn_amd import ops
    x, gy = torch.zeros(0, 64, device="cuda"), torch.zeros(0, 32, device="cuda")
    gw, gb = _routed(lambda: ops.linear_weight_grad(x, gy, want_bias=True), P.wgrad_route(0, 64, 32), "zero rows")
    assert gw.shape == (32, 64) and float(gw.abs().sum()) == 0.0 and float(gb.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
def _grads_close(got, want, what):
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert g_ is not None, f"{what}: gradient {i} is missing"
        _assert_close(g_, w_.double(), GRAD_TOL, f"{what} gradient {i}")


@pytest.mark.parametrize("rows,k,n_out,env", [(300, 50, 37, {}), (3000, 64, 96, {}), (300, 128, 128, {FORCE: "1"}),
                                             (2049, 128, 128, {FORCE: "1"})])
def test_dense_linear_autograd_matches_float64(rows, k, n_out, env, monkeypatch):
    from ptgnn_amd import dense
    _set_env(monkeypatch, env)
    torch.manual_seed(rows + k)
    lin = torch.nn.Linear(k, n_out)
    x, gout = torch.randn(rows, k), torch.randn(rows, n_out)
    ref = copy.deepcopy(lin).double()
    x1 = x.double().requires_grad_(True)
    ref(x1).backward(gout.double())
    lin = lin.cuda()
    x2 = x.cuda().requires_grad_(True)
    y = dense.linear(x2, lin.weight, lin.bias)
    _assert_close(y.detach(), ref(x.double()).detach(), TOL, "dense.linear forward")
    y.backward(gout.cuda())
    _grads_close([x2.grad, lin.weight.grad, lin.bias.grad], [x1.grad, ref.weight.grad, ref.bias.grad],
                 f"dense.linear {rows}x{k}->{n_out}")


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows,k,n_out,env", [(300, 52, 36, {}), (3000, 64, 96, {}), (300, 128, 128, {FORCE: "1"})])
def test_dense_linear_act_dropout_autograd_matches_float64(rows, k, n_out, env, act, p, monkeypatch):
    """The reference applies the mask the node kept (its fourth saved tensor) with the scale 1 / (1 - p)."""
    from ptgnn_amd import dense
    _set_env(monkeypatch, env)
    torch.manual_seed(rows + k)
    lin = torch.nn.Linear(k, n_out)
    x, gout = torch.randn(rows, k), torch.randn(rows, n_out)
    ref = copy.deepcopy(lin).double()
    lin = lin.cuda()
    x2 = x.cuda().requires_grad_(True)
    out = dense.linear_act_dropout(x2, lin.weight, lin.bias, act, p, True)
    assert out is not None
    keep = out.grad_fn.saved_tensors[3]
    assert (keep is None) == (p == 0.0)
    x1 = x.double().requires_grad_(True)
    y1 = _act64(ref(x1), act)
    if keep is not None:
        assert 0.5 < float(keep.float().mean()) < 0.9
        y1 = y1 * keep.cpu().double() * (1.0 / (1.0 - p))
    _assert_close(out.detach(), y1.detach(), TOL, "linear_act_dropout forward")
    y1.backward(gout.double())
    out.backward(gout.cuda())
    _grads_close([x2.grad, lin.weight.grad, lin.bias.grad], [x1.grad, ref.weight.grad, ref.bias.grad],
                 f"linear_act_dropout {rows}x{k}->{n_out} act={act} p={p}")


def test_dense_linear_act_dropout_declines_widths_off_four():
    from ptgnn_amd import dense
    lin = torch.nn.Linear(50, 37).cuda()
    assert dense.linear_act_dropout(torch.randn(8, 50, device="cuda"), lin.weight, lin.bias, "tanh", 0.1, True) is None


@pytest.mark.parametrize("n,m,hd,bias,env", [(3000, 64, 96, True, {}), (300, 128, 128, True, {FORCE: "1"}), (2049, 128, 128, True, {FORCE: "1"}),
                                            (300, 50, 36, True, {}), (300, 64, 96, False, {}), (300, 24, 18, True, {}),
                                            (300, 128, 128, True, {FORCE: "1", GRU_RING: "1"})])
def test_dense_gru_cell_autograd_matches_float64_and_follows_an_optimizer_step(n, m, hd, bias, env, monkeypatch):
    """d a, d h and every parameter gradient against torch float64 CPU autograd; after an optimizer step the second
    backward must use the new weights (the transposed-weight cache is keyed on the parameter's version).  The float64
    copy takes the stepped fp32 weights over, so both sides differentiate the same parameters."""
    from ptgnn_amd import dense
    _set_env(monkeypatch, env)
    torch.manual_seed(n + m + hd)
    cell = torch.nn.GRUCell(m, hd, bias=bias)
    a, h, gout = torch.randn(n, m), torch.randn(n, hd), torch.randn(n, hd)
    ref = copy.deepcopy(cell).double()
    cell = cell.cuda()
    opt = torch.optim.SGD(cell.parameters(), lr=0.05)
    for step in range(2):
        a1, h1 = a.double().requires_grad_(True), h.double().requires_grad_(True)
        a2, h2 = a.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
        opt.zero_grad()
        ref.zero_grad()
        y1 = ref(a1, h1)
        y2 = dense.gru_cell(cell, a2, h2)
        what = f"dense.gru_cell n={n} m={m} hd={hd} bias={bias} step={step}"
        _assert_close(y2.detach(), y1.detach(), TOL, what + " forward")
        y1.backward(gout.double())
        y2.backward(gout.cuda())
        _grads_close([a2.grad, h2.grad] + [q.grad for q in cell.parameters()],
                     [a1.grad, h1.grad] + [q.grad for q in ref.parameters()], what)
        before = [q.detach().clone() for q in cell.parameters()]
        opt.step()
        assert all(not torch.equal(q.detach(), b) for q, b in zip(cell.parameters(), before))
        ref.load_state_dict({key: v.detach().cpu().double() for key, v in cell.state_dict().items()})


# ---------------------------------------------------------------------------------------------------------------------
# completeness
# ---------------------------------------------------------------------------------------------------------------------
def test_zz_every_route_name_was_asserted_through_a_launch_counter(monkeypatch):
    """Runs last.  Every route name of the restated dispatches has been asserted from the launch counters by the tests
    above; a route a partial selection of this file left out is run here on a small witness first."""
    from ptgnn_amd import ops
    cus = _cus()
    for k, n_out, env, mode in P.LINEAR_SHAPES:
        name = P.linear_route(33, k, n_out, env=env, cus=cus, mode=mode).name
        if name not in SEEN:
            x, w, b = P.linear_case(33, k, n_out)
            _set_env(monkeypatch, env)
            with _mode(mode):
                got = _routed(lambda: ops.linear(x.cuda(), w.cuda(), b.cuda()), name, "witness")
            _assert_close(got, P.linear_ref(x, w, b), TOL, f"witness {name}")
    for m, hd in P.GRU_SHAPES:
        for env in ({}, {GRU_RING: "1"}):
            name = P.gru_route(33, m, hd, env=env)
            if name not in SEEN:
                case = P.gru_case(33, m, hd)
                _set_env(monkeypatch, env)
                got = _routed(lambda: ops.gru_cell(*[t.cuda() for t in case]), name, "witness")
                _assert_close(got, P.gru_ref(*case)[0], TOL, f"witness {name}")
    for k in P.WGRAD_STREAM_WIDTHS + P.WGRAD_TILE_WIDTHS[:1]:
        for n_out in P.WGRAD_STREAM_WIDTHS:
            if P.wgrad_route(33, k, n_out) not in SEEN:
                _wgrad_check(33, k, n_out)
    missing = set(P.ALL_ROUTES) - SEEN
    assert not missing, f"routes never asserted through a launch counter: {sorted(missing)}"
