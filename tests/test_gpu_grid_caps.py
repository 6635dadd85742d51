"""Every capped launch grid past its cap, on the MI355X.

Many kernels cap their grid and cover the rest of the work with a grid-stride loop; that loop takes a second trip only
when the work exceeds cap x work per workgroup.  A second trip that is skipped, or that runs with a wrong stride, leaves
rows unwritten or counted twice.  Every case here is the smallest input past its threshold (tests/grid_caps.py: the
table, the case builders, the restatements; tests/test_grid_caps_cpu.py holds them against the source text), carries
witness work in the second trip, asserts its size against the table before it launches, and hands the entry points
that take an output buffer one pre-filled with NaN -- an unwritten row then shows as NaN, not as stale zeros.

Bars: integer kernels and copies are compared bit for bit; sums of small integers (all partial sums below 2^24) are
exact whatever the fold order; float results are held to the project's bars (tests/agg_paths.py TOL = 1e-5, the
gradient bar 2e-5 x max(1, |want|), the attributed rule where fp32 itself drifts), always against float64."""
import ctypes

import numpy as np
import pytest
import torch

import agg_paths as AP
import grid_caps as G
from helpers import to_cuda_adj

pytestmark = pytest.mark.gpu

I32 = torch.int32
DEV = "cuda"


def _past(case, name, per_wg=None):
    thr = G.threshold(name, per_wg)
    assert case["size"] > thr and all(p >= thr for p in case["witness"]), (name, case["size"], thr)
    return thr


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# 1. index guard
# ---------------------------------------------------------------------------------------------------------------------
def test_index_guard_counts_the_bad_ids_of_its_second_trip():
    """k_validate (ptgnn_amd_validate_indices: 2048 workgroups x 256 ids).  The plan build counts its bad ids inside its
    own kernels, so the 700,000 ids reach k_validate through the library entry, in ONE call, and are counted into the
    device's accumulator -- the one `ops.check_indices(sync=True)` reads and reports.  The three bad ids all sit at
    positions >= 524,288: a negative one at the first id of the second trip, one == N, and the very last id."""
    from ptgnn_amd import _lib, ops
    c = G.validate_case()
    _past(c, "validate")
    lib = _lib.load()
    ops.check_indices(sync=True)                                   # clean slate
    acc = ops._bad_accumulator(ops._device_state(torch.device(DEV)))
    for ids, planted in ((c["clean"], 0), (c["bad"], len(c["planted"]))):
        d = ids.to(DEV)
        _lib.check(lib.ptgnn_amd_validate_indices(d.data_ptr(), d.shape[0], c["num_nodes"], acc.data_ptr(), _stream(d)),
                   "ptgnn_amd_validate_indices")
        if planted == 0:
            ops.check_indices(sync=True)                           # a clean list of the same size raises nothing
        else:
            with pytest.raises(_lib.PtgnnAmdError, match=rf"^{planted} node id"):
                ops.check_indices(sync=True)
    ops.check_indices(sync=True)                                   # the raise cleared the accumulator
    # the plan build's own guard on the same ids (700,000 edges of one type, the ids as sources)
    dst = c["clean"].to(DEV)
    ops.build_plan([(c["bad"].to(DEV), dst)], c["num_nodes"])
    with pytest.raises(_lib.PtgnnAmdError, match=r"^3 node id"):
        ops.check_indices(sync=True)
    good = ops.build_plan([(c["clean"].to(DEV), dst)], c["num_nodes"])
    ops.check_indices(sync=True)
    assert int(good.rowptr[-1]) == c["size"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. shard index
# ---------------------------------------------------------------------------------------------------------------------
def test_shard_index_of_a_table_past_the_cap_equals_the_torch_bookkeeping():
    """k_shard_mark / k_shard_remap (8192 workgroups x 256 edges per table): one rank whose destination range holds all
    2,200,000 edges of one table, sources over three ranks; bit for bit against the torch-op chain, as
    test_shard_index_kernels_equal_the_torch_bookkeeping does.  Two remote sources occur only in the second trip (its
    first edge and the table's last edge): they must be in the halo list and their edges remapped onto their rows."""
    from ptgnn_amd import sharded
    c = G.shard_case()
    thr = _past(c, "shard")
    mine = to_cuda_adj(c["adj"])
    a = sharded.ShardedGraph.build_local(mine, c["ranges"], c["rank"], overlap=True, use_hip_index=True)
    b = sharded.ShardedGraph.build_local(mine, c["ranges"], c["rank"], overlap=True, use_hip_index=False)
    assert a.recv_splits == b.recv_splits and a.n_halo == b.n_halo
    assert torch.equal(a.need_ids, b.need_ids)
    for (sa, da), (sb, db) in zip(a.local_adj, b.local_adj):
        assert torch.equal(sa, sb) and torch.equal(da, db)
    for (sa, da), (sb, db) in zip(a.adj_own + a.adj_halo, b.adj_own + b.adj_halo):
        assert torch.equal(sa, sb) and torch.equal(da, db)
    need = a.need_ids.cpu()
    ls = a.local_adj[0][0].cpu()
    for pos, wid in zip(c["witness"], c["witness_ids"]):
        slot = torch.nonzero(need == wid).flatten()
        assert slot.numel() == 1, f"remote source {wid} (edge {pos} >= {thr}) is missing from the halo list"
        assert int(ls[pos]) == a.n_local + int(slot)
    # the whole remap against a searchsorted restatement (need_ids is sorted)
    src, dst = c["adj"][0]
    lo, hi = c["ranges"][c["rank"]]
    own = (src >= lo) & (src < hi)
    want = torch.where(own, src - lo, a.n_local + torch.searchsorted(need, src))
    assert torch.equal(ls, want) and torch.equal(a.local_adj[0][1].cpu(), dst - lo)


# ---------------------------------------------------------------------------------------------------------------------
# 3. unique sources
# ---------------------------------------------------------------------------------------------------------------------
def test_unique_sources_of_a_plan_past_the_cap_equal_the_numpy_bookkeeping(monkeypatch):
    """k_uniq_mark / k_uniq_remap (8192 x 256 CSR slots; the remap's stride is gridDim.x - 1 workgroups): edge counts
    [1,500,000, 700,000] over 70,001 nodes, bit for bit against numpy -- the distinct sources per type, slot_row of
    every slot (searchsorted per type), the counts.  Two (type, source) pairs exist only in the second trip."""
    from ptgnn_amd import ops
    c = G.unique_case()
    thr = _past(c, "uniq")
    monkeypatch.setattr(ops._device_state(DEV).uniq_backoff, "steps", 0)
    ops.clear_plan_cache()
    plan = ops.plan_for(to_cuda_adj(c["adj"]), c["num_nodes"])
    assert plan.num_edges == c["size"] > thr
    uq = plan.unique_messages()
    assert uq is not None
    col = plan.col[: plan.num_edges].cpu().numpy()
    want, rows, counts = G.unique_ref(c["adj"], c["num_nodes"], plan.type_bits, col)
    np.testing.assert_array_equal(uq.counts.cpu().numpy(), counts)
    assert uq.rows(wait=True) == counts[-1]
    for t, (got, _) in enumerate(uq.adjacency()):
        np.testing.assert_array_equal(got.cpu().numpy(), want[t])
    got_rows = uq.slot_row[: plan.num_edges].cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(got_rows[thr:], rows[thr:])          # the second trip, named on its own
    np.testing.assert_array_equal(got_rows, rows)
    off = np.cumsum([0] + [len(w) for w in want])
    for slot, (t, s) in zip(c["witness"], c["witness_pairs"]):
        assert s in want[t] and got_rows[slot] == off[t] + np.searchsorted(want[t], s)
    ops.clear_plan_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 4. gather_rows
# ---------------------------------------------------------------------------------------------------------------------
def _gather_rows_into(x, idx, out):
    from ptgnn_amd import _lib, ops
    x = ops._rowmajor(x)
    rc = _lib.load().ptgnn_amd_gather_rows_f32(x.data_ptr(), ops._ld(x), idx.data_ptr(), idx.shape[0], x.shape[1],
                                               out.data_ptr(), out.stride(0), _stream(out))
    _lib.check(rc, "ptgnn_amd_gather_rows_f32")


@pytest.mark.parametrize("form", ["dim4", "dim6", "dim260", "slice"])
def test_gather_rows_past_the_cap_equals_indexing(form):
    """k_gather_rows (8192 workgroups x 4 rows, a wave per row): 32,768 + 3 rows.  dim 4 copies float4s, dim 6 scalars,
    dim 260 gives lane 0 a second column step (c = 256), `slice` is an unaligned column slice of a wider table (scalar
    copies at dim 4, ld 9).  Must equal x[idx] exactly; the output starts as NaN."""
    from ptgnn_amd import ops
    c = G.gather_rows_case()
    thr = _past(c, "gather_rows")
    g = torch.Generator().manual_seed(40)
    if form == "slice":
        x = torch.randn(c["table_rows"], 9, generator=g).to(DEV)[:, 1:5]
        assert x.data_ptr() % 16 != 0 and x.stride(0) == 9
    else:
        x = torch.randn(c["table_rows"], int(form[3:]), generator=g).to(DEV)
    idx = c["idx"].to(DEV)
    out = _nan(c["size"], x.shape[1])
    _gather_rows_into(x, idx, out)
    want = x.cpu()[c["idx"]]
    got = out.cpu()
    assert torch.equal(got[thr:].view(I32), want[thr:].view(I32)), "rows of the second trip"
    assert torch.equal(got.view(I32), want.view(I32))
    assert torch.equal(ops.gather_rows(x, idx).view(I32), out.view(I32))      # the entry the layers call


# ---------------------------------------------------------------------------------------------------------------------
# 5. generic spread
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", sorted(G.SPREAD_SHAPES))
def test_generic_spread_past_the_cap_equals_the_index_restatement(dim):
    """k_segment_spread (65,536 workgroups x 256 items).  dim 3 selects k_segment_spread<false> (a scalar item per slot
    and column: 5,592,406 slots), dim 260 k_segment_spread<true> (an item per float4: 258,112 slots); widths 64, 128 and
    256 take k_segment_spread_rows, which has no capped grid.  With and without an arg, exactly, output pre-filled with
    NaN.  The last slot's row names it as the winner of every column, so the second trip's items carry gradient."""
    from ptgnn_amd import _lib, ops
    c = G.spread_case(dim)
    _past(c, "spread")
    plan = ops.build_plan(to_cuda_adj(c["adj"]), c["num_nodes"])
    E = plan.num_edges
    assert E == c["slots"] and G.spread_items(dim, E) == c["size"]
    np.testing.assert_array_equal(plan.perm[:E].cpu().numpy(), c["perm"])      # the stable sort the restatement assumes
    grad = torch.randn(c["num_nodes"], dim, generator=torch.Generator().manual_seed(50 + dim)) + 3.0   # no zero entry
    gd, argd = grad.to(DEV), c["arg"].to(DEV)
    assert gd.data_ptr() % 16 == 0 and argd.data_ptr() % 16 == 0
    lib = _lib.load()
    for arg in (None, argd):
        out = _nan(E, dim)
        rc = lib.ptgnn_amd_segment_spread_f32(gd.data_ptr(), dim, arg.data_ptr() if arg is not None else None,
                                              plan.slot_rows().data_ptr(), plan.perm.data_ptr(), E, dim, out.data_ptr(),
                                              dim, _stream(out))
        _lib.check(rc, "ptgnn_amd_segment_spread_f32")
        want = G.spread_ref(grad.numpy(), c["arg"].numpy() if arg is not None else None, c["perm"], c["rows"])
        got = out.cpu().numpy()
        last = c["perm"][E - 1]
        np.testing.assert_array_equal(got[last], grad.numpy()[c["rows"][E - 1]])   # the second trip's slot, with gradient
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
        del out
    assert torch.equal(ops.segment_spread(gd, argd, plan).cpu().view(I32), torch.from_numpy(want).view(I32))


# ---------------------------------------------------------------------------------------------------------------------
# 6. row epilogue backward
# ---------------------------------------------------------------------------------------------------------------------
def _dist(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


@pytest.mark.parametrize("flags", sorted(G.ROW_EPILOGUE_FLAGS))
@pytest.mark.parametrize("rows,dim", G.ROW_EPILOGUE_SHAPES)
def test_row_epilogue_backward_past_the_cap_against_float64(rows, dim, flags):
    """k_row_epilogue_backward (2048 workgroups x 256 / LPR rows): a few rows past the cap of every lane geometry; 130
    and 301 are the scalar CH = 4 / CH = 8 routes (widths off four above 64) that no other test launches, forward and
    backward.  grad_x within 2e-5 x max(1, |want|) of float64 (the project's gradient bar); grad_gamma / grad_beta are
    column sums over up to 32,785 rows, where fp32 torch itself drifts: the attributed bar, no further from float64
    than twice the fp32 reference's own distance (tol 2e-5 x max(1, |float64|)).  Outputs start as NaN."""
    from ptgnn_amd import _lib, ops
    c = G.row_epilogue_case(rows, dim, flags)
    thr = _past(c, "row_epilogue_backward", c["per_wg"])
    lib, ln, fl = _lib.load(), "ln" in flags, G.ROW_EPILOGUE_FLAGS[flags]
    y64, gx64, gg64, gb64 = G.row_epilogue_ref(c["x"], c["gy"], c["gamma"], c["beta"], flags, torch.float64)
    y32, gx32, gg32, gb32 = G.row_epilogue_ref(c["x"], c["gy"], c["gamma"], c["beta"], flags, torch.float32)
    x, gy = c["x"].to(DEV), c["gy"].to(DEV)
    gamma, beta = (c["gamma"].to(DEV), c["beta"].to(DEV)) if ln else (None, None)
    y = ops.row_epilogue(x, fl, gamma, beta)
    print(f"\n    {rows}x{dim} {flags} route {G.row_epilogue_route(dim)}: y |fp32-f64|={_dist(y32, y64):.3e} "
          f"|got-f64|={_dist(y, y64):.3e}")
    assert AP.attributed_ok(y, y32, y64, tol=AP.TOL, scale=max(1.0, float(y64.abs().max())))
    gx = _nan(rows, dim)
    gg, gb = (_nan(dim), _nan(dim)) if ln else (None, None)
    ws_bytes = int(lib.ptgnn_amd_row_epilogue_workspace_bytes(rows, dim)) if ln else 0
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    rc = lib.ptgnn_amd_row_epilogue_backward_f32(x.data_ptr(), dim, gy.data_ptr(), dim, rows, dim, fl,
                                                 gamma.data_ptr() if ln else None, 1e-5, gx.data_ptr(), dim,
                                                 gg.data_ptr() if ln else None, gb.data_ptr() if ln else None,
                                                 ws.data_ptr() if ln else None, ws_bytes, _stream(gx))
    _lib.check(rc, "ptgnn_amd_row_epilogue_backward_f32")
    bar = 2e-5 * max(1.0, float(gx64.abs().max()))
    print(f"    grad_x |fp32-f64|={_dist(gx32, gx64):.3e} |got-f64|={_dist(gx, gx64):.3e} bar={bar:.3e}; second trip "
          f"rows {thr}..{rows - 1}: |got-f64|={_dist(gx[thr:], gx64[thr:]):.3e}")
    assert bool(torch.isfinite(gx[thr:]).all()), "rows of the second trip were not written"
    assert _dist(gx, gx64) <= bar
    if ln:
        for name, got, w32, w64 in (("grad_gamma", gg, gg32, gg64), ("grad_beta", gb, gb32, gb64)):
            print(f"    {name} |fp32-f64|={_dist(w32, w64):.3e} |got-f64|={_dist(got, w64):.3e}")
            assert AP.attributed_ok(got, w32, w64, tol=2e-5, scale=max(1.0, float(w64.abs().max()))), name
    got3 = ops.row_epilogue_backward(x, gy, fl, gamma)
    assert torch.equal(got3[0].view(I32), gx.view(I32)) and (not ln or torch.equal(got3[1].view(I32), gg.view(I32)))


# ---------------------------------------------------------------------------------------------------------------------
# 7. PNA long rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 6])
def test_pna_long_rows_past_the_cap_against_float64(M):
    """k_pna_long_rows / k_pna_bwd_long_rows (1024 workgroups x 256 rows scanned): N = 262,144 + 300, rows of 257 and
    300 in-edges at row 5, on both sides of row 262,144 and at row N - 1, 3,000 background edges, every other row empty.
    PNA is row-wise, so the float64 / fp32 restatement (agg_paths.pna_ref) runs on the non-empty rows renumbered --
    EVERY non-empty row, first trip and second -- and the empty rows must be exact zeros.  M = 4 (float4 columns) and
    M = 6 (scalar).  The attributed bar of tests/test_gpu_pna.py; two calls give equal bits."""
    from ptgnn_amd import ops
    from ptgnn_amd.layers import PnaMessageAggregation
    c = G.pna_case(M)
    thr = _past(c, "pna_long")
    N, live = c["num_nodes"], c["live"]
    agg = PnaMessageAggregation()
    m = c["messages"].to(DEV).requires_grad_(True)
    t = c["targets"].to(DEV)
    before = ops.launch_counts(aggregation=True)
    out = agg(messages=m, message_targets=t, num_nodes=N)
    assert ops.launches_since(before).get("pna_aggregate") == 1
    with torch.no_grad():
        again = agg(messages=m.detach(), message_targets=t, num_nodes=N)
    assert torch.equal(out.detach().view(I32), again.view(I32)), "two calls differ"
    gout = torch.zeros(N, 15 * M, device=DEV)
    gout[live.to(DEV)] = c["gout"].to(DEV)
    (out * gout).sum().backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        mr = c["messages"].to(dt).requires_grad_(True)
        o = AP.pna_ref(mr, c["compact"], live.shape[0], 1.0)
        (o * c["gout"].to(dt)).sum().backward()
        refs[dt] = (o.detach(), mr.grad)
    out_c = out.detach().cpu()
    empty = torch.ones(N, dtype=torch.bool)
    empty[live] = False
    assert float(out_c[empty].abs().max()) == 0.0 and bool(empty[thr:].any())
    got = out_c[live]
    second = live >= thr
    assert int(second.sum()) >= len(c["witness"])
    print(f"\n    M={M}: out |fp32-f64|={_dist(refs[torch.float32][0], refs[torch.float64][0]):.3e} "
          f"|got-f64|={_dist(got, refs[torch.float64][0]):.3e} (second trip rows: "
          f"{_dist(got[second], refs[torch.float64][0][second]):.3e}); grad |fp32-f64|="
          f"{_dist(refs[torch.float32][1], refs[torch.float64][1]):.3e} |got-f64|={_dist(m.grad, refs[torch.float64][1]):.3e}")
    assert AP.attributed_ok(got[second], refs[torch.float32][0][second], refs[torch.float64][0][second]), "second trip"
    assert AP.attributed_ok(got, refs[torch.float32][0], refs[torch.float64][0])
    sc = max(1.0, float(refs[torch.float64][1].abs().max()))
    late = torch.isin(c["targets"], torch.tensor(c["witness"]))
    assert AP.attributed_ok(m.grad[late.to(DEV)], refs[torch.float32][1][late], refs[torch.float64][1][late], scale=sc)
    assert AP.attributed_ok(m.grad, refs[torch.float32][1], refs[torch.float64][1], scale=sc)


# ---------------------------------------------------------------------------------------------------------------------
# 8. hub list and long rows of the CSR aggregation
# ---------------------------------------------------------------------------------------------------------------------
def _plant_maxima(plan, msgs, hub_row, thr):
    """Read the plan's hub list and give column 1 its one 4 in the chunk of list entry `thr` (the first entry of the hub
    launch's second trip) and column 2 its one 4 in the chunk of the last entry: a second trip that is skipped loses
    both maxima.  Returns the number of entries."""
    count = int(plan.hub_count.item())
    entries = plan.hub_entries[:count].cpu()
    assert count > thr and bool((entries[:, 1] == hub_row).all())
    rowptr, perm = plan.rowptr.cpu(), plan.perm.cpu().long()
    beg, end = int(rowptr[hub_row]), int(rowptr[hub_row + 1])
    for col, e in ((1, thr), (2, count - 1)):
        chunk = int(entries[e, 0])
        lo, hi = max(beg, chunk * G.K_HUB_CHUNK), min(end, (chunk + 1) * G.K_HUB_CHUNK)
        assert lo < hi
        msgs[perm[(lo + hi) // 2], col] = 4.0
    return count


def _check_exact(plan, c, msgs, what):
    """sum, max (with and without the arg output), min and mean of `msgs` over `plan` against float64: sum, max and
    min exactly (small integers), the arg against agg_paths.first_winner, mean to TOL.  Returns the launches made."""
    from ptgnn_amd import ops
    N, M, E = c["num_nodes"], msgs.shape[1], plan.num_edges
    dst = c["adj"][0][1]
    y = msgs.to(DEV)
    perm = plan.perm[:E].cpu().long()
    before = ops.launch_counts(aggregation=True)
    want = G.segment_ref64(msgs, dst, N, "sum")
    out = _nan(N, M)
    ops.gather_reduce(y, plan, M, "sum", type_bits=0, col=plan.perm, out=out)
    assert torch.equal(out.cpu().double(), want), (what, "sum", torch.nonzero((out.cpu().double() != want).any(1))[:8])
    for reduce in ("max", "min"):
        val, arg = AP.first_winner(msgs, dst, N, reduce)
        out = _nan(N, M)
        ops.gather_reduce(y, plan, M, reduce, type_bits=0, col=plan.perm, out=out)
        assert torch.equal(out.cpu().double(), val.double()), (what, reduce)
        out = _nan(N, M)
        _, slot = ops.gather_reduce(y, plan, M, reduce, type_bits=0, col=plan.perm, out=out, return_arg=True)
        assert torch.equal(out.cpu().double(), val.double()), (what, reduce, "with arg")
        slot = slot.cpu().long()
        edge = torch.where(slot >= 0, perm[slot.clamp(min=0)], torch.full_like(slot, E))
        assert torch.equal(edge, arg), (what, reduce, "arg", torch.nonzero((edge != arg).any(1))[:8])
    out = _nan(N, M)
    ops.gather_reduce(y, plan, M, "mean", type_bits=0, col=plan.perm, out=out)
    err = float((out.cpu().double() - G.segment_ref64(msgs, dst, N, "mean")).abs().max())
    assert err <= AP.TOL, (what, "mean", err)
    torch.cuda.synchronize()
    assert int(plan.hub_tickets(M).abs().sum()) == 0
    return ops.launches_since(before)


def test_hub_list_longer_than_the_hub_grid_on_one_stream():
    """8(a) k_hub_chunks, the dedicated launch (min(chunks, 1024) workgroups stride the hub list): E < 2^21, one row of
    1,100,000 in-edges = more than 1,024 (chunk, row) entries, M = 4.  With an arg output (the training form) the hub
    list is walked by the dedicated launch; without one the main kernel's first 32 workgroups walk it (the fused form:
    the same loop at a stride of 32).  Small-integer messages: sum, max and min exactly, mean to TOL."""
    from ptgnn_amd import ops
    c = G.hub_case()
    thr = _past(c, "hub_chunks")
    plan = ops.build_plan(to_cuda_adj(c["adj"]), c["num_nodes"])
    assert plan.num_edges < (1 << 21) and plan.may_have_hubs()
    msgs = G.small_int_messages(plan.num_edges, 4, seed=80)
    count = _plant_maxima(plan, msgs, c["hub_row"], thr)
    assert count == c["size"]
    ran = _check_exact(plan, c, msgs, "hub launch")
    assert ran.get("k_gather_reduce") == 6, ran


def test_side_stream_hub_chunks_and_long_rows_past_their_caps():
    """8(b) E >= 2^21 by its real size: k_hub_chunks on the side stream (a hub of 1,200,000 in-edges: more than 1,024
    entries) and k_long_rows on the second side stream (2048 workgroups x 256 rows scanned; N = 524,288 + 600, long
    rows of 257 to 2,048 in-edges on both sides of row 524,288 and at row N - 1) in one graph, M = 4.  Small-integer
    messages: sum, max and min exactly, mean to TOL.  The hub sits at row N - 2, past the 262,144 rows of k_max_degree's
    first trip, and is the plan's maximum degree."""
    from ptgnn_amd import _lib, ops
    c = G.side_stream_case()
    thr = _past(c, "long_rows")
    assert c["hub_size"] > G.threshold("hub_chunks") and c["max_degree_row"] >= G.threshold("max_degree")
    adj = to_cuda_adj(c["adj"])
    plan = ops.build_plan(adj, c["num_nodes"])
    assert plan.num_edges >= (1 << 21) and plan.may_have_hubs()
    deg = (plan.rowptr[1:] - plan.rowptr[:-1]).cpu().long()
    assert torch.equal(deg, c["deg"])
    assert all(AP.K_LONG_ROW < int(deg[r]) <= AP.HUB_THRESHOLD for r in c["witness"]) and min(c["witness"]) == thr
    msgs = G.small_int_messages(plan.num_edges, 4, seed=81)
    count = _plant_maxima(plan, msgs, c["hub_row"], G.threshold("hub_chunks"))
    assert count == c["hub_size"]
    ran = _check_exact(plan, c, msgs, "side streams")
    assert ran.get("k_gather_reduce") == 6, ran
    # k_max_degree (1024 workgroups x 256 rows): the library entry with a max_degree scalar, as ops.build_plan calls it
    lib = _lib.load()
    (s, d), N, E = adj[0], c["num_nodes"], plan.num_edges
    rowptr = torch.empty(N + 1, dtype=I32, device=DEV)
    col, perm = torch.empty(E, dtype=I32, device=DEV), torch.empty(E, dtype=I32, device=DEV)
    maxdeg = torch.full((1,), -1, dtype=I32, device=DEV)
    ws_bytes = lib.ptgnn_amd_csr_workspace_bytes(E, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    one = ctypes.c_void_p * 1
    rc = lib.ptgnn_amd_csr_build(ctypes.cast(one(s.data_ptr()), ctypes.c_void_p),
                                 ctypes.cast(one(d.data_ptr()), ctypes.c_void_p),
                                 ctypes.cast((ctypes.c_int64 * 1)(E), ctypes.c_void_p), 1, N, 0, 0, rowptr.data_ptr(),
                                 col.data_ptr(), perm.data_ptr(), maxdeg.data_ptr(), 0, None, None, None,
                                 ops._plan_control(torch.device(DEV)).data_ptr(), ws.data_ptr(), ws_bytes, _stream(ws))
    _lib.check(rc, "ptgnn_amd_csr_build")
    assert int(maxdeg.item()) == int(c["deg"].max()) == 1_200_000
    assert torch.equal(rowptr, plan.rowptr) and torch.equal(perm, plan.perm[:E])


# ---------------------------------------------------------------------------------------------------------------------
# 9. char-CNN kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_char_embed_past_the_cap_against_float64():
    """k_char_embed (65,536 workgroups x 256 items of 4 columns): B R dim / 4 just above 16,777,216.  The float64
    restatement of tests/char_embedder_cases.py (`_conv` over the one-hot input, ReLU) on every row of the second trip
    and on as many rows of the first (the frame has 65,799 rows of 1020 columns: the CPU reference of all of them would
    dominate), to the bar of tests/test_gpu_char_embedder.py (attributed, TOL x max(1, |float64|)); and EVERY element
    bit for bit against the same three-term fp32 sum (bias + tap 0 + tap 1, in that order) taken with torch on the
    device.  The frame starts as NaN."""
    from char_embedder_cases import _conv
    from ptgnn_amd import ops
    c = G.char_embed_case()
    thr = _past(c, "char")
    B, R, C, W, dim = c["B"], c["R"], c["C"], c["W"], c["dim"]
    assert ops.char_embed_supported(C, W, dim)
    table, bias, chars = G.char_table(c["w1"]).to(DEV), c["b1"].to(DEV), c["chars"].to(DEV)
    frame = _nan(B * R, dim)
    a1 = ops.char_embed(chars, table, bias, W, out=frame)
    assert a1.data_ptr() == frame.data_ptr() and bool(torch.isfinite(frame[c["first_row"]:]).all())
    taps = chars.unfold(1, W, 1).reshape(B * R, W)                               # [B R, W] character of every tap
    for lo in range(0, B * R, 16384):                                           # by row blocks: no second frame
        same = bias + table[taps[lo:lo + 16384, 0]]
        for k in range(1, W):
            same = same + table[k * C + taps[lo:lo + 16384, k]]
        assert torch.equal(torch.relu(same).view(I32), frame[lo:lo + 16384].view(I32)), f"rows from {lo}"
    del same
    tail = torch.arange(c["first_row"] // R, B)                                  # samples that own second-trip rows
    head = torch.arange(0, tail.shape[0])
    mid = torch.randint(0, B, (tail.shape[0],), generator=torch.Generator().manual_seed(90))
    got = frame.cpu().reshape(B, R, dim)
    for name, pick in (("second trip", tail), ("first samples", head), ("random samples", mid)):
        ch = c["chars"][pick]
        refs = [torch.relu(_conv(torch.eye(C, dtype=dt)[ch], c["w1"].to(dt), c["b1"].to(dt)))
                for dt in (torch.float32, torch.float64)]
        scale = max(1.0, float(refs[1].abs().max()))
        print(f"\n    {name}: |fp32-f64|={_dist(refs[0], refs[1]):.3e} |got-f64|={_dist(got[pick], refs[1]):.3e}")
        assert AP.attributed_ok(got[pick], refs[0], refs[1], AP.TOL, scale), name


def test_window_max_past_the_cap_is_exact():
    """k_window_max (65,536 x 256 items; scalar columns at dim = 255): B dim just above 16,777,216, two rows per sample,
    small integers (ties: the lowest position wins).  Max and arg exactly against the float64 restatement."""
    from ptgnn_amd import ops
    c = G.window_max_case()
    _past(c, "char")
    B, R = c["B"], c["R"]
    out, arg = ops.window_max(c["x"].to(DEV), 0, B, R, R, return_arg=True)
    best, first = G.window_max_ref(c["x"], B, R, R)
    assert bool((first[c["first_row"]:] == 1).any()) and bool((first[c["first_row"]:] == 0).any())
    assert torch.equal(out.cpu().double()[c["first_row"]:], best[c["first_row"]:]), "samples of the second trip"
    assert torch.equal(out.cpu().double(), best) and torch.equal(arg.cpu().long(), first.long())


def test_window_max_backward_past_the_cap_is_exact():
    """k_window_max_backward (65,536 x 256 items; scalar columns at dim = 255): B R dim just above 16,777,216.  Exactly
    grad[b, d] at row arg[b, d] and zeros elsewhere; the frame starts as NaN."""
    from ptgnn_amd import ops
    c = G.window_max_backward_case()
    _past(c, "char")
    B, R, dim = c["B"], c["R"], c["dim"]
    frame = _nan(B * R, dim)
    gx = ops.window_max_backward(c["grad"].to(DEV), c["arg"].to(DEV), R, out=frame)
    want = G.window_max_backward_ref(c["grad"], c["arg"], R)
    got = gx.cpu()
    assert torch.equal(got[c["first_row"]:].view(I32), want[c["first_row"]:].view(I32)), "rows of the second trip"
    assert torch.equal(got.view(I32), want.view(I32))


# ---------------------------------------------------------------------------------------------------------------------
# 10. the plan build's small capped kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_of_more_than_64_edge_types_past_the_pack_cap_equals_numpy():
    """k_pack (4096 workgroups x 256 edges of one table of 64 edge types): 65 edge types whose first 64 hold
    1,048,576 + 362 edges.  rowptr, col and perm bit for bit against a stable numpy sort."""
    from ptgnn_amd import ops
    c = G.pack_case()
    _past(c, "pack")
    plan = ops.build_plan(to_cuda_adj(c["adj"]), c["num_nodes"])
    E = plan.num_edges
    perm, rows, col = G.plan_ref(c["adj"], plan.type_bits)
    assert plan.type_bits == 7 and E == perm.shape[0]
    np.testing.assert_array_equal(plan.perm[:E].cpu().numpy(), perm)
    np.testing.assert_array_equal(plan.col[:E].cpu().numpy().astype(np.int64), col)
    want_ptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=c["num_nodes"]))]
    np.testing.assert_array_equal(plan.rowptr.cpu().numpy(), want_ptr)


def test_edge_free_plan_past_the_zero_fill_cap():
    """k_zero_rowptr (1024 workgroups x 256 entries): a plan without edges over 262,144 + 300 rows."""
    from ptgnn_amd import ops
    c = G.zero_rowptr_case()
    _past(c, "zero_rowptr")
    filler = torch.full((c["num_nodes"] + 1,), -1, dtype=I32, device=DEV)       # the block the plan's rowptr may reuse
    del filler
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    plan = ops.build_plan([(e, e)], c["num_nodes"])
    assert plan.rowptr.shape[0] == c["size"] and int(plan.rowptr.abs().max()) == 0


def test_hub_list_of_a_sorted_index_past_its_cap():
    """k_hub_list (2048 workgroups x 256 rows) through ops.plan_from_sorted_index: 524,288 + 600 segments with hub
    segments at 7, at the first row of the second trip and at the last row.  The list holds exactly their (chunk, row)
    entries (in any order); the segment sums of all-ones are the segment sizes."""
    from ptgnn_amd import ops
    c = G.hub_list_case()
    _past(c, "hub_list")
    plan = ops.plan_from_sorted_index(c["index"].to(DEV), c["num_segments"])
    count = int(plan.hub_count.item())
    got = sorted(map(tuple, plan.hub_entries[:count].cpu().tolist()))
    assert got == sorted(c["entries"])
    ones = torch.ones(c["index"].shape[0], 4, device=DEV)
    out = _nan(c["num_segments"], 4)
    ops.gather_reduce(ones, plan, 4, "sum", type_bits=0, col=plan.perm, out=out)
    assert torch.equal(out[:, 0].cpu().long(), c["deg"])
