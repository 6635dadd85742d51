"""The tail split of the streaming GEMMs (ptgnn_amd/csrc/stream_gemm.hip): the last `count % 8` units of a workgroup's run
are shared between its waves as sub-units -- in `k_stream_gru` one accumulator group {r}, {z}, {n_i, h_n} each.  A
sub-unit keeps the K chain of each accumulator, so the results must stay bit for bit what whole units give, and within the
dense tests' bound of float64 (tests/dense_paths.py TOL: 1e-5 * max(1, |want|inf)).  The same split by 32 x 32 output
blocks was built for `k_stream_linear` / `k_stream_edge`, passed the cases below and measured slower
(profiles/tail_split_notes.md): those kernels keep whole units, and their cases stay as tests of every run-tail geometry
against the tile kernels (`ops.set_gemm_mode("tile")`), bit for bit.

Sizes come from the launch geometry, so that one workgroup's run has `count % 8` = 0, 1, 2, 3, 4, 5 and 7, fewer than 8
units (the run is all tail) and exactly one; the last unit is always ragged (rows % 32 = 27):
  * dense kernels: `dense_runs` gives cus / column-slabs runs, so rows = 32 * runs * count - 5 puts `count` units into
    every run (Linear K = 128 -> 128: one slab; GRU M = H = 128: four feature tiles; M = 128, H = 256: eight, K = 384,
    whose slab leaves no room for the exchange area -- the unsplit path);
  * edge kernels: with 32 * count - 5, 40 and 0 edges the table gives the first type one workgroup of `count` units up to
    count = 13 (two workgroups of 7 and 8 units at count = 15) and the second type one workgroup of two units.

`gru_cell` cannot be compared with the tile kernel by `torch.equal`, with or without the split: the tile GRU evaluates
its gates with libm's expf / tanhf (dense_f32.hip), the streaming GRU with the hardware exponential and reciprocal.
Measured on the MI355X at M = H = 128, 20 475 rows: 1 062 603 of 2 620 800 elements differ, by at most 7.2e-7 (9.6e-7 over
all cases of this file), on the whole-unit build as on this one.  So the GRU cases assert equal bits against what IS comparable: the training launch of
the same kernel (`gru_cell_train`: it keeps whole units and runs the same gate math), and that launch's `gh_n` output
(the h_n accumulator + bias, no transcendental) against the tile kernel's."""
import pytest
import torch

import dense_paths as P
from dense_paths import FORCE, TOL

pytestmark = pytest.mark.gpu

COUNTS = (8, 9, 10, 11, 12, 13, 15, 5, 1)      # units per run: count % 8 = 0 1 2 3 4 5 7, all tail, one unit


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tile(fn):
    from ptgnn_amd import ops
    prev = ops.set_gemm_mode("tile")
    try:
        return fn()
    finally:
        ops.set_gemm_mode(prev)


def _streamed(fn, counter):
    """Run fn on the streaming route; `counter` must have moved by exactly one launch."""
    from ptgnn_amd import ops
    before = ops.launch_counts()
    out = fn()
    since = ops.launches_since(before)
    assert since.get(counter, 0) == 1, f"expected one {counter} launch, the library counted {since}"
    return out


def _close(got, want64, what):
    bound = TOL * max(1.0, float(want64.abs().max()))
    err = float((got.double() - want64).abs().max())
    print(f"{what}: max |err| vs float64 {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max error {err:.3e} beyond {bound:.3e}"


def _same(got, want, what):
    diff = int((got != want).sum())
    print(f"{what}: {diff} elements differ")
    if diff:
        idx = torch.nonzero(got != want)[0].tolist()
        raise AssertionError(f"{what}: {diff} elements differ, first at {idx}: {got[tuple(idx)].item()!r} != "
                             f"{want[tuple(idx)].item()!r}")


# ---------------------------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_linear_tail_blocks_equal_the_tile_kernel(count, monkeypatch):
    from ptgnn_amd import ops
    monkeypatch.setenv(FORCE, "1")             # below the streaming route's size floor at these row counts
    cus = _cus()
    rps, run_len = P.dense_runs(cus * count, 1, cus)
    assert (rps, run_len) == (cus, count)
    rows = 32 * cus * count - 5
    x, w, b = (t.cuda() for t in P.linear_case(rows, 128, 128, seed=count))
    addend = torch.randn(rows, 128, generator=torch.Generator().manual_seed(count)).cuda()
    pre = x.double() @ w.double().t()
    # bias
    got = _streamed(lambda: ops.linear(x, w, b), "k_stream_linear")
    _close(got, pre + b.double(), f"linear count {count}")
    _same(got, _tile(lambda: ops.linear(x, w, b)), f"linear count {count} vs tile")
    # bias with tanh (both kernels: the hardware exponential of dense_common.h)
    got = _streamed(lambda: ops.linear(x, w, b, act="tanh"), "k_stream_linear")
    _close(got, torch.tanh(pre + b.double()), f"linear tanh count {count}")
    _same(got, _tile(lambda: ops.linear(x, w, b, act="tanh")), f"linear tanh count {count} vs tile")
    # the addend form (streaming launch only: in tile mode the GEMM is followed by torch's add, the same sum)
    got = _streamed(lambda: ops.linear_add(x, w, addend, b), "k_stream_linear")
    _close(got, pre + b.double() + addend.double(), f"linear_add count {count}")
    _same(got, _tile(lambda: ops.linear_add(x, w, addend, b)), f"linear_add count {count} vs tile")


# ---------------------------------------------------------------------------------------------------------------------
# gru_cell
# ---------------------------------------------------------------------------------------------------------------------
def _gru_checks(n, m, hd, count, what, strided_out=False):
    from ptgnn_amd import ops
    a, h, w_ih, w_hh, b_ih, b_hh = (t.cuda() for t in P.gru_case(n, m, hd, seed=count))
    want = P.gru_ref(a, h, w_ih, w_hh, b_ih, b_hh)[0].cuda()
    if strided_out:
        buf = torch.full((n, 256), -7.0, device="cuda")
        out = buf[:, 64:64 + hd]
        got = _streamed(lambda: ops.gru_cell(a, h, w_ih, w_hh, b_ih, b_hh, out=out), "k_stream_gru")
        assert got.data_ptr() == out.data_ptr() and out.stride(0) == 256
        assert bool((buf[:, :64] == -7.0).all()) and bool((buf[:, 64 + hd:] == -7.0).all())
    else:
        got = _streamed(lambda: ops.gru_cell(a, h, w_ih, w_hh, b_ih, b_hh), "k_stream_gru")
    _close(got, want, what)
    # the training launch of the same kernel keeps whole units: the split accumulator groups must give its bits
    whole, gates = _streamed(lambda: ops.gru_cell_train(a, h, w_ih, w_hh, b_ih, b_hh), "k_stream_gru")
    _same(got, whole, what + " vs the whole-unit launch")
    # and that launch meets the tile kernel bit for bit where no transcendental stands in between: gh_n = h W_hn^T + b_hn
    tile, tile_gates = _tile(lambda: ops.gru_cell_train(a, h, w_ih, w_hh, b_ih, b_hh))
    _same(gates[:, 3 * hd:], tile_gates[:, 3 * hd:], what + ": gh_n vs tile")
    _close(tile, want, what + " (tile)")
    print(f"{what}: {int((got != tile).sum())} of {got.numel()} elements differ from the tile kernel's (libm gates), "
          f"max {float((got - tile).abs().max()):.3e}")


@pytest.mark.parametrize("count", COUNTS)
def test_gru_tail_groups_equal_the_tile_kernel(count):
    cus = _cus()
    rps, run_len = P.dense_runs(cus // 4 * count, 4, cus)
    assert (rps, run_len) == (cus // 4, count)
    _gru_checks(32 * (cus // 4) * count - 5, 128, 128, count, f"gru count {count}")


def test_gru_wide_state_keeps_whole_units_and_the_same_bits():
    cus = _cus()
    rps, run_len = P.dense_runs(cus // 8 * 11, 8, cus)
    assert (rps, run_len) == (cus // 8, 11)
    _gru_checks(32 * (cus // 8) * 11 - 5, 128, 256, 11, "gru H = 256 count 11")


def test_gru_tail_groups_store_into_a_strided_out():
    cus = _cus()
    _gru_checks(32 * (cus // 4) * 10 - 5, 128, 128, 10, "gru strided out count 10", strided_out=True)


# ---------------------------------------------------------------------------------------------------------------------
# edge_linear / edge_linear_shared
# ---------------------------------------------------------------------------------------------------------------------
def _edge_case(count, use_dst, seed, distinct_sources=False):
    H = M = 128
    n = 4096
    K = 2 * H if use_dst else H
    g = torch.Generator().manual_seed(seed)
    adj = []
    for c in (32 * count - 5, 40, 0):
        src = torch.randperm(n, generator=g)[:c] if distinct_sources else torch.randint(0, n, (c,), generator=g)
        adj.append((src, torch.randint(0, n, (c,), generator=g)))
    x = torch.randn(n, H, generator=g)
    ws = [torch.randn(M, K, generator=g) / K ** 0.5 for _ in adj]
    return n, adj, x, ws


def _edge_ref(x, adj, ws, use_dst):
    x = x.double()
    return torch.cat([(torch.cat([x[s], x[d]], -1) if use_dst else x[s]) @ w.double().t() for (s, d), w in zip(adj, ws)])


@pytest.mark.parametrize("use_dst", [False, True], ids=["src", "src_dst"])
@pytest.mark.parametrize("count", COUNTS)
def test_edge_linear_tail_blocks_equal_the_tile_kernel(count, use_dst):
    from ptgnn_amd import ops
    n, adj, x, ws = _edge_case(count, use_dst, 100 * count + use_dst)
    cadj = [(s.cuda(), d.cuda()) for s, d in adj]
    cx, cws = x.cuda(), [w.cuda() for w in ws]
    got = _streamed(lambda: ops.edge_linear(cx, cadj, cws, use_dst), "k_stream_edge")
    assert got.shape == (32 * count - 5 + 40, 128)
    _close(got, _edge_ref(cx, cadj, cws, use_dst), f"edge_linear count {count} use_dst {use_dst}")
    _same(got, _tile(lambda: ops.edge_linear(cx, cadj, cws, use_dst)), f"edge_linear count {count} use_dst {use_dst} vs tile")


@pytest.mark.parametrize("count", COUNTS)
def test_edge_linear_shared_tail_blocks_equal_the_tile_kernel(count, monkeypatch):
    from ptgnn_amd import ops
    monkeypatch.setattr(ops, "UNIQUE_MIN_EDGES", 0)
    monkeypatch.setattr(ops, "UNIQUE_MIN_SAVING", -1.0)
    monkeypatch.setattr(ops._device_state("cuda").uniq_backoff, "steps", 0)
    n, adj, x, ws = _edge_case(count, False, 300 + count, distinct_sources=True)   # one message row per edge
    cadj = [(s.cuda(), d.cuda()) for s, d in adj]
    cx, cws = x.cuda(), [w.cuda() for w in ws]
    ops.clear_plan_cache()
    uq = ops.plan_for(cadj, n).unique_messages()
    assert uq is not None
    rows_adj = [(s, s) for s, _ in uq.adjacency()]
    total = sum(int(s.shape[0]) for s, _ in rows_adj)
    assert [int(s.shape[0]) for s, _ in rows_adj] == [32 * count - 5, 40, 0] and uq.rows(wait=True) == total
    got = _streamed(lambda: ops.edge_linear_shared(cx, uq, cws), "k_stream_edge_shared")[:total]
    _close(got, _edge_ref(cx, rows_adj, cws, False), f"edge_linear_shared count {count}")
    _same(got, _tile(lambda: ops.edge_linear(cx, rows_adj, cws, False)), f"edge_linear_shared count {count} vs tile")
    ops.clear_plan_cache()
