"""The per-segment ops on minibatches of MANY small segments (tests/segment_batches.py): the chunk table of
csrc/segment_chunks.h past the first wave and the first 1024-segment step of its scan, the binary search over hundreds of
entries with runs of empty segments, the window table past 256 graphs, the two head merges past one chunk / slot per
thread -- against float64 on the attributed bar of tests/agg_paths.py, and bit for bit against the same segments run as a
shorter batch -- and the same entry points on column slices of wider NaN-filled buffers (leading dimension != width, a
base that is not 16-byte aligned)."""
import functools
import math
import types
from unittest import mock

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import segment_batches as SB
import test_gpu_attention_pool as attention_pool_tests
import test_gpu_graphnorm as graphnorm_tests
import test_gpu_heads as head_tests
from agg_paths import TOL, attributed_ok
from ptgnn_amd import heads, ops, reduceops as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
INF = float("inf")
EPS = 1e-10                  # GraphNorm's, as tests/test_gpu_graphnorm.py
SCORE_VECTORS = 5
WIDTHS = (64, 6)             # the float4 and the scalar variant of every chunked kernel


def bar(got, want32, exact, what):
    """agg_paths.attributed_ok relative to max(1, max |float64|) over the finite float64 entries; -inf entries must sit at
    the same positions and nothing may be nan.  Prints each figure first."""
    got, want32, exact = (torch.as_tensor(t).detach().double().cpu() for t in (got, want32, exact))
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    assert torch.equal(got == -INF, exact == -INF), what
    finite = torch.isfinite(exact)
    if not bool(finite.any()):
        return True
    got, want32, exact = got[finite], want32[finite], exact[finite]
    assert bool(torch.isfinite(got).all()), what
    scale = max(1.0, float(exact.abs().max()))
    print(f"    {what}: |got-fp32|={float((got - want32).abs().max()):.3e} |got-f64|={float((got - exact).abs().max()):.3e} "
          f"|fp32-f64|={float((want32 - exact).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


def make_plan(idx, segments, shuffled):
    return ops.plan_for([(idx, idx)], segments) if shuffled else ops.plan_from_sorted_index(idx, segments)


# ---------------------------------------------------------------------------------------------------------------------
# the four chunk-table families: a case (inputs on the device), the kernels' outputs, the restatement's
# ---------------------------------------------------------------------------------------------------------------------
def base_case(counts, D, shuffled, seed):
    idx = SB.index_of(counts, shuffled, seed)
    c = types.SimpleNamespace(counts=list(counts), D=D, shuffled=shuffled, idx=idx.to(DEV), n=int(idx.shape[0]),
                              segments=len(counts), rows={}, segs={}, shared={})
    c.plan = make_plan(c.idx, c.segments, shuffled)
    c.empty = torch.tensor([k == 0 for k in counts], device=DEV)
    return c, torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def leaf(t, dt):
    """A CPU copy of `t` in `dt` that autograd differentiates.  The restatements run on the CPU: its index_add adds in
    element order, so a reference -- and with the deterministic kernels the verdict of a test -- is the same every run
    (the GPU's adds with float atomics in an order that varies)."""
    return t.detach().cpu().to(dt).clone().requires_grad_(True)


def host(t, dt=None):
    return t.detach().cpu() if dt is None else t.detach().cpu().to(dt)


def weighted_case(counts, D, shuffled, seed, heads_=None):
    c, g = base_case(counts, D, shuffled, seed)
    c.rows["x"] = randn(g, c.n, D)
    c.segs["gout"] = randn(g, c.segments, D)
    c.shared["w"] = randn(g, 1, D, scale=1.0 / math.sqrt(D))
    return c


def weighted_run(c, **over):
    t = {**c.rows, **c.segs, **c.shared, **over}
    out = ops.weighted_pool(t["x"], t["w"], c.plan)
    gx, gw = ops.weighted_pool_backward(t["x"], t["w"], c.idx, t["gout"])
    return {"grad_x": gx}, {"out": out}, {"grad_w": gw}


def weighted_ref(c, dt):
    x, w = leaf(c.rows["x"], dt), leaf(c.shared["w"], dt)
    out = SB.ref_weighted(x, host(c.idx), c.segments, w)
    out.backward(host(c.segs["gout"], dt))
    return {"out": out.detach(), "grad_x": x.grad, "grad_w": w.grad.reshape(-1)}


def attention_case(counts, D, shuffled, seed, heads_=4):
    c, g = base_case(counts, D, shuffled, seed)
    c.heads = heads_
    c.rows["x"] = randn(g, c.n, D)
    c.segs["u"] = randn(g, c.segments, heads_, D, scale=1.0 / math.sqrt(D))
    c.segs["gpool"] = randn(g, c.segments, heads_, D)
    return c


def attention_run(c, **over):
    t = {**c.rows, **c.segs, **over}
    pooled, stats = ops.attention_pool(t["x"], t["u"], c.plan)
    gx, gu = ops.attention_pool_backward(t["x"], t["u"], c.plan, pooled, stats, t["gpool"])
    return {"grad_x": gx}, {"pooled": pooled, "stats": stats, "grad_u": gu}, {}


def attention_ref(c, dt):
    x, u = leaf(c.rows["x"], dt), leaf(c.segs["u"], dt)
    pooled, top, lse = SB.ref_attention_pool(x, host(c.idx), c.segments, u)
    (pooled * host(c.segs["gpool"], dt)).sum().backward()
    # the kernel's stats block: max | log-sum-exp per head, 0 for a segment without elements
    stats = torch.cat([top, lse.detach()], dim=1)
    stats = torch.where(host(c.empty).unsqueeze(1), torch.zeros_like(stats), stats)
    return {"pooled": pooled.detach(), "stats": stats, "grad_x": x.grad, "grad_u": u.grad}


def scores_case(counts, D, shuffled, seed, heads_=None):
    c, g = base_case(counts, D, shuffled, seed)
    c.rows["y"] = randn(g, c.n, D)
    c.rows["gs"] = randn(g, c.n, SCORE_VECTORS)
    c.segs["v"] = randn(g, c.segments, SCORE_VECTORS, D, scale=1.0 / math.sqrt(D))
    c.segs["gl"] = randn(g, c.segments, SCORE_VECTORS)
    return c


def scores_run(c, **over):
    t = {**c.rows, **c.segs, **over}
    scores, lse = ops.segment_scores(t["y"], t["v"], c.plan)
    gy, gv = ops.segment_scores_backward(t["y"], t["v"], c.plan, scores, lse, t["gs"], t["gl"])
    return {"scores": scores, "grad_y": gy}, {"lse": lse, "grad_v": gv}, {}


def scores_ref(c, dt):
    y, v = leaf(c.rows["y"], dt), leaf(c.segs["v"], dt)
    idx, live = host(c.idx), ~host(c.empty)
    s = (v[idx] * y.unsqueeze(1)).sum(-1)
    l = SB.segment_lse(s, idx, c.segments)
    ((s * host(c.rows["gs"], dt)).sum() + (l[live] * host(c.segs["gl"], dt)[live]).sum()).backward()
    return {"scores": s.detach(), "lse": l.detach(), "grad_y": y.grad, "grad_v": v.grad}


def graphnorm_case(counts, D, shuffled, seed, heads_=None):
    c, g = base_case(counts, D, shuffled, seed)
    c.rows["x"] = randn(g, c.n, D)
    c.rows["gy"] = randn(g, c.n, D)
    for name in ("gamma", "alpha"):
        c.shared[name] = (0.5 + torch.rand(1, D, generator=g)).to(DEV)
    c.shared["bias"] = randn(g, 1, D)
    return c


def graphnorm_run(c, **over):
    t = {**c.rows, **c.shared, **over}
    y, mean = ops.graph_norm(t["x"], t["gamma"], t["alpha"], t["bias"], EPS, c.plan, with_mean=True)
    gx, gg, ga, gb = ops.graph_norm_backward(t["x"], t["gy"], t["gamma"], t["alpha"], EPS, mean, c.plan)
    return {"y": y, "grad_x": gx}, {"mean": mean}, {"grad_gamma": gg, "grad_alpha": ga, "grad_bias": gb}


def graphnorm_ref(c, dt):
    x = leaf(c.rows["x"], dt)
    p = [leaf(c.shared[k], dt) for k in ("gamma", "alpha", "bias")]
    y = SB.ref_graphnorm(x, host(c.idx), *p, EPS)
    y.backward(host(c.rows["gy"], dt))
    return {"y": y.detach(), "mean": SB.ref_graph_means(x.detach(), host(c.idx), c.segments), "grad_x": x.grad,
            "grad_gamma": p[0].grad.reshape(-1), "grad_alpha": p[1].grad.reshape(-1), "grad_bias": p[2].grad.reshape(-1)}


FAMILIES = {"weighted_pool": (weighted_case, weighted_run, weighted_ref),
            "attention_pool": (attention_case, attention_run, attention_ref),
            "segment_scores": (scores_case, scores_run, scores_ref),
            "graph_norm": (graphnorm_case, graphnorm_run, graphnorm_ref)}
# what a family's outputs hold for a segment WITHOUT elements, exactly
EMPTY_VALUES = {"out": 0.0, "pooled": 0.0, "stats": 0.0, "grad_u": 0.0, "lse": -INF, "grad_v": 0.0, "mean": 0.0}


def seed_of(family, G, phase, D, shuffled):
    return 1000 * sorted(FAMILIES).index(family) + 7 * G + 3 * phase + D + (500 if shuffled else 0)


def check_family_against_float64(family, c, got):
    """The kernels' outputs `got` (the three dicts of a family's run) of case `c`: exact values on the segments without
    elements, no nan, and the attributed bar against the fp32 and the float64 restatement."""
    _, _, ref = FAMILIES[family]
    rows, segs, whole = got
    flat = {**rows, **segs, **whole}
    for name, t in flat.items():
        assert not bool(torch.isnan(t).any()), name
        if name.startswith("grad"):
            assert bool(torch.isfinite(t).all()), name
    for name, t in segs.items():
        want = EMPTY_VALUES[name]
        assert bool((t[c.empty] == want).all()), (name, "segments without elements")
        assert bool(torch.isfinite(t[~c.empty]).all()), name               # -inf exactly on the empty segments
    want32, exact = ref(c, torch.float32), ref(c, torch.float64)
    assert set(flat) == set(exact)
    for name, t in flat.items():
        assert bar(t, want32[name], exact[name], f"{family} {name}"), name


# ---------------------------------------------------------------------------------------------------------------------
# 3a. every batch, sorted and shuffled, against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("G,phase", SB.CHUNK_BATCHES, ids=[f"G{G}p{p}" for G, p in SB.CHUNK_BATCHES])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_chunk_table_ops_on_many_segments_against_float64(family, G, phase, shuffled, D):
    make, run, _ = FAMILIES[family]
    counts = SB.sizes(G, phase) + [0] * SB.TRAILING_EMPTY
    c = make(counts, D, shuffled, seed_of(family, G, phase, D, shuffled), 8 if G == 2100 else 4)
    assert c.segments == G + SB.TRAILING_EMPTY and int(c.empty.sum()) >= SB.TRAILING_EMPTY + G // 3
    if shuffled:
        assert not bool((c.idx[1:] >= c.idx[:-1]).all())
    check_family_against_float64(family, c, run(c))


# ---------------------------------------------------------------------------------------------------------------------
# 3b. a segment's value is a fixed function of its own rows: the first segments of the longest batch, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def prefix_of(c, segments):
    """The first `segments` segments of a sorted case as a case of their own: the same tensors, sliced."""
    assert not c.shuffled
    m = sum(c.counts[:segments])
    p = types.SimpleNamespace(counts=c.counts[:segments], D=c.D, shuffled=False, idx=c.idx[:m], n=m, segments=segments,
                              rows={k: v[:m] for k, v in c.rows.items()}, segs={k: v[:segments] for k, v in c.segs.items()},
                              shared=c.shared, empty=c.empty[:segments])
    p.plan = ops.plan_from_sorted_index(p.idx, segments)
    return p


@functools.lru_cache(maxsize=None)
def longest_batch(family, D):
    make, run, _ = FAMILIES[family]
    c = make(SB.sizes(2100, 0) + [0] * SB.TRAILING_EMPTY, D, False, seed_of(family, 2100, 0, D, False), 8)
    return c, run(c)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("segments", [1024, 65])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_first_segments_of_2100_have_the_bits_of_a_batch_of_their_own(family, segments, D):
    c, (rows, segs, _) = longest_batch(family, D)
    p = prefix_of(c, segments)
    assert p.counts == SB.sizes(segments, 0) and 0 < p.n < c.n
    alone_rows, alone_segs, _ = FAMILIES[family][1](p)
    for name, t in alone_rows.items():
        assert t.shape[0] == p.n and torch.equal(rows[name][:p.n], t), name
    for name, t in alone_segs.items():
        assert t.shape[0] == segments and torch.equal(segs[name][:segments], t), name


# ---------------------------------------------------------------------------------------------------------------------
# 3c. the window table and block attention beyond 256 graphs
# ---------------------------------------------------------------------------------------------------------------------
HEADS, DK, DV = 3, 6, 10
WINDOW_ROWS = (3, 40)


def window_counts(G):
    return SB.sizes(G, 0) + [0] * SB.TRAILING_EMPTY


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("max_num_nodes", WINDOW_ROWS)
@pytest.mark.parametrize("G", [G for G, _ in SB.WINDOW_BATCHES])
def test_window_table_of_many_graphs(G, max_num_nodes, shuffled):
    counts = window_counts(G)
    idx = SB.index_of(counts, shuffled, seed=G)
    n, segments = int(idx.shape[0]), len(counts)
    table = ops.attention_windows(make_plan(idx.to(DEV), segments, shuffled), max_num_nodes).cpu()
    want = SB.window_offsets(counts, max_num_nodes)
    bound = -(-n // max_num_nodes) + segments
    assert segments > 256 and len(want) - 1 < bound                        # past the scan's first step; a tail to fill
    assert table.shape == (bound + 1,) and table.dtype == torch.int32
    assert table[:len(want)].tolist() == want                              # entry for entry
    assert bool((table[len(want):] == n).all())                             # the tail


@functools.lru_cache(maxsize=None)
def attention_reference(G, max_num_nodes):
    """(kqv, gout, {dtype: (out, grad_kqv)}) on the CPU, computed once per configuration and never modified."""
    counts = window_counts(G)
    g = torch.Generator().manual_seed(40 + G + max_num_nodes)
    n = sum(counts)
    kqv = torch.randn(n, HEADS * (2 * DK + DV), generator=g)
    gout = torch.randn(n, HEADS * DV, generator=g)
    res = {}
    for dt in (torch.float32, torch.float64):
        k = kqv.to(dt).clone().requires_grad_(True)
        out = SB.ref_attention(k, counts, max_num_nodes, HEADS, DK, DV)
        out.backward(gout.to(dt))
        res[dt] = (out.detach(), k.grad)
    return kqv, gout, res


def gpu_attention(kqv, gout, counts, max_num_nodes):
    idx = SB.index_of(counts, False).to(DEV)
    windows = ops.attention_windows(ops.plan_from_sorted_index(idx, len(counts)), max_num_nodes)
    out, lse = ops.block_attention(kqv, windows, max_num_nodes, HEADS, DK, DV)
    grad = ops.block_attention_backward(kqv, out, lse, gout, windows, max_num_nodes, HEADS, DK, DV)
    return out, lse, grad


@pytest.mark.parametrize("max_num_nodes", WINDOW_ROWS)
@pytest.mark.parametrize("G", [G for G, _ in SB.WINDOW_BATCHES])
def test_block_attention_over_many_graphs(G, max_num_nodes):
    counts = window_counts(G)
    kqv, gout, res = attention_reference(G, max_num_nodes)
    kqv, gout = kqv.to(DEV), gout.to(DEV)
    out, lse, grad = gpu_attention(kqv, gout, counts, max_num_nodes)
    assert bool(torch.isfinite(lse).all())
    assert bar(out, res[torch.float32][0], res[torch.float64][0], "out")
    assert bar(grad, res[torch.float32][1], res[torch.float64][1], "grad_kqv")
    m = sum(counts[:256])                                                  # the graphs of the scan's first step, alone
    alone = gpu_attention(kqv[:m], gout[:m], counts[:256], max_num_nodes)
    assert 0 < m and (m < kqv.shape[0]) == (G > 257)                       # graph 257 of the 257 is empty: only the tail moves
    for whole, part in zip((out, lse, grad), alone):
        assert torch.equal(whole[:m], part)


# ---------------------------------------------------------------------------------------------------------------------
# 3d. the head merges beyond one chunk / one slot per thread
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
@pytest.mark.parametrize("rows", [32768, 32769, 70001])
def test_logit_merge_with_runs_of_one_two_and_three_chunks(rows, mode):
    assert -(-(-(-rows // 128)) // 256) == {32768: 1, 32769: 2, 70001: 3}[rows]
    head_tests.check_logit_loss_kernel(rows, 3, mode, torch.Generator().manual_seed(rows))


@pytest.mark.parametrize("G", [G for G, _ in SB.CANDIDATE_BATCHES])
def test_candidate_merge_with_runs_of_two_and_three_slots(G):
    D = 64
    x, w, cand_idx, slot_idx, cand_slot, correct, counts = SB.candidate_slots_batch(G, D, seed=6000 + G)
    slots, Cn = len(counts), int(cand_idx.shape[0])
    assert -(-slots // 256) == {257: 2, 700: 3}[G] and not bool((cand_slot[1:] >= cand_slot[:-1]).all())
    skipped = counts.count(0) + 1                                          # the empty slots' -1 and the index past the end
    x, w, cand_idx, slot_idx, cand_slot, correct = (t.to(DEV) for t in (x, w, cand_idx, slot_idx, cand_slot, correct))
    gen = torch.Generator().manual_seed(G)
    cot = torch.randn(Cn, generator=gen).to(DEV)
    g = torch.tensor(1.75, device=DEV)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    metrics = ops.head_metrics_block(DEV)
    before = ops.launch_counts(heads=True)
    loss, scores, lse, argmax = heads.candidate_loss(xl, wl, cand_idx, slot_idx, cand_slot, correct, metrics)
    (loss * g + (scores * cot).sum()).backward()
    assert ops.launches_since(before) == {"candidate_scores": 1, "candidate_scores_backward": 1}
    on_host = [host(t) for t in (x, w, cand_idx, slot_idx, cand_slot, correct, cot, g)]
    r32, r64 = SB.candidate_ref(*on_host, torch.float32), SB.candidate_ref(*on_host, torch.float64)
    assert bar(loss, r32[0], r64[0], "loss")
    assert bar(scores, r32[1], r64[1], "scores")
    assert bar(lse, r32[2], r64[2], "lse")                                 # -inf exactly on the empty slots
    empty = torch.tensor([k == 0 for k in counts], device=DEV)
    assert torch.equal(lse == -INF, empty) and bool((argmax[empty] == Cn).all())
    # arg-max positions: the float64 winner, unless its margin is within the fp32 error of a score
    s64, arg, arg64, slot_of = r64[1].detach().cpu(), argmax.cpu(), r64[3].cpu(), cand_slot.cpu()
    margin = 1e-4 * max(1.0, float(s64.abs().max()))
    for slot in range(slots):
        if counts[slot] == 0:
            continue
        own = torch.nonzero(slot_of == slot).flatten()
        best = own[s64[own] >= s64[own].max() - margin]
        assert int(arg[slot]) in best.tolist(), slot
        if best.numel() == 1:
            assert int(arg[slot]) == int(arg64[slot])
    assert bar(xl.grad, r32[4].grad, r64[4].grad, "d x")
    assert bar(wl.grad, r32[5].grad, r64[5].grad, "d w")
    hits = int((arg == correct.cpu()).sum())
    assert 0 < hits < slots
    assert metrics.tolist() == [hits, slots, skipped, 0]
    _, _, _, _, totals = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot,
                                              ops.build_plan([(cand_slot, cand_slot)], slots), w, correct)
    assert totals[1:6].tolist() == [slots, hits, skipped, 0, Cn]


# ---------------------------------------------------------------------------------------------------------------------
# 3e. one pass through the modules with 1025 segments
# ---------------------------------------------------------------------------------------------------------------------
def test_multihead_reducer_with_1025_samples():
    counts = SB.sizes(1025, 0)
    y = attention_pool_tests.check_against_float64(64, 4, False, counts, 1.0)       # counts its two fused launches
    empty = torch.tensor([k == 0 for k in counts] + [True], device=DEV)
    assert y.shape[0] == 1026 and not bool(y[empty].any())


def test_graphnorm_layer_with_1025_graphs():
    counts = SB.sizes(1025, 0)
    assert counts[-1] > 0                                                  # the layer takes the graph count from the map
    graphnorm_tests.check_against_float64(64, counts)                      # one launch forward, one backward


def test_weighted_sum_reducer_with_1025_samples():
    D, counts = 64, SB.sizes(1025, 0) + [0] * SB.TRAILING_EMPTY
    segments = len(counts)
    g = torch.Generator().manual_seed(77)
    idx = SB.index_of(counts, True, seed=78).to(DEV)
    x, gout = randn(g, idx.shape[0], D), randn(g, segments, D)
    torch.manual_seed(79)
    module = R.WeightedSumVarSizedElementReduce(D).to(DEV)
    xl = x.clone().requires_grad_(True)
    with mock.patch.object(ops, "weighted_pool", wraps=ops.weighted_pool) as forward, \
            mock.patch.object(ops, "weighted_pool_backward", wraps=ops.weighted_pool_backward) as backward:
        y = module(R.ElementsToSummaryRepresentationInput(xl, idx, segments))
        y.backward(gout)
    assert forward.call_count == 1 and backward.call_count == 1
    res = {}
    for dt in (torch.float32, torch.float64):
        xr, wr = leaf(x, dt), leaf(module.score_weight, dt)
        out = SB.ref_weighted(xr, host(idx), segments, wr)
        out.backward(host(gout, dt))
        res[dt] = {"y": out.detach(), "x": xr.grad, "w": wr.grad}
    got = {"y": y, "x": xl.grad, "w": module.score_weight.grad}
    for name, t in got.items():
        assert bar(t, res[torch.float32][name], res[torch.float64][name], name), name
    assert not bool(y[torch.tensor([k == 0 for k in counts], device=DEV)].any())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the same entry points on column slices of wider NaN-filled buffers
# ---------------------------------------------------------------------------------------------------------------------
VIEW_COUNTS = ([129, 1, 0, 57], [1])
VIEW_KINDS = ("aligned", "off")
COPY_OPS = ("clone", "copy_", "_to_copy", "contiguous")


def as_view(t, kind):
    """`t` [n, D] as a column slice of a wider buffer filled with nan: "aligned" keeps the base on 16 bytes and, at a D in
    fours, the leading dimension in fours; "off" puts the base 4 bytes off and makes the leading dimension odd."""
    n, D = t.shape
    pad, at = (8, 4) if kind == "aligned" else (3, 1)
    buf = torch.full((n, D + pad), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[:, at:at + D]
    view.copy_(t)
    assert view.stride(0) == D + pad and view.data_ptr() % 16 == (0 if kind == "aligned" else 4)
    assert ops._ld(view) == D + pad                                       # also for one row: the leading dimension the
    return view                                                            # kernel gets is the buffer's


def fresh(t):
    """`t` in an allocation of its own with the leading dimension D (`.contiguous()` returns a one-row view itself)."""
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    out.copy_(t)
    assert out.stride(0) == t.shape[1] and out.data_ptr() % 16 == 0
    return out


def float4_rows(t):
    """The predicate every chunked entry point applies to a row operand: float4 loads when the width, the leading
    dimension and the base allow them."""
    return t.shape[1] % 4 == 0 and ops._ld(t) % 4 == 0 and t.data_ptr() % 16 == 0


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.ops.append((func.overloadpacket.__name__, [tuple(t.shape) for t in outs if isinstance(t, torch.Tensor)]))
        return out


def recorded_copies(fn, shapes):
    """(result of fn(), the copies of a tensor of one of `shapes` made while it ran)."""
    with _Recorder() as rec:
        out = fn()
    return out, [(name, s) for name, outs in rec.ops for s in outs if name in COPY_OPS and s in shapes]


def all_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def no_nan(tensors):
    return all(not bool(torch.isnan(t).any()) for t in tensors)


# the row operands each wrapper passes with a leading dimension of their own
VIEWED = {"weighted_pool": ("x", "gout"), "attention_pool": ("x",), "segment_scores": ("y",), "graph_norm": ("x", "gy")}


@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("counts", VIEW_COUNTS, ids=["four_segments", "one_row"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_chunk_table_ops_read_views_through_their_leading_dimension(family, counts, D, kind):
    make, run, _ = FAMILIES[family]
    c = make(counts, D, len(counts) > 1, seed_of(family, len(counts), 9, D, kind == "off"), 4)
    tensors = {**c.rows, **c.segs}
    views = {k: as_view(tensors[k], kind) for k in VIEWED[family]}
    plain = {k: fresh(tensors[k]) for k in VIEWED[family]}
    got, copies = recorded_copies(lambda: run(c, **views), {tuple(v.shape) for v in views.values()})
    flat = {k: t for part in got for k, t in part.items()}
    assert no_nan(flat.values())                                           # a nan is a read outside the view
    # which kernel variant the view takes, from the entry point's own predicate
    vector_plain = all(float4_rows(t) for t in plain.values())
    vector_view = all(float4_rows(t) for t in views.values())
    assert vector_plain == (D % 4 == 0) and vector_view == (D % 4 == 0 and kind == "aligned")
    # GraphNorm alone copies an operand float4 loads cannot read when the width allows them (a one-row operand has no
    # other layout to be copied into: it takes the scalar kernels)
    copied = family == "graph_norm" and D % 4 == 0 and kind == "off" and c.n > 1
    assert len(copies) == (3 if copied else 0), copies                     # x forward, x and grad_y backward
    if copied or vector_view == vector_plain:
        want = run(c, **plain)
        assert all_equal(flat, {k: t for part in want for k, t in part.items()})
    else:
        check_family_against_float64(family, c, got)


def small_attention_case(counts):
    g = torch.Generator().manual_seed(60 + len(counts))
    n = sum(counts)
    return randn(g, n, HEADS * (2 * DK + DV)), randn(g, n, HEADS * DV)


@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("counts", VIEW_COUNTS, ids=["four_segments", "one_row"])
def test_block_attention_reads_views_through_their_leading_dimension(counts, kind):
    kqv, gout = small_attention_case(counts)
    shapes = {tuple(kqv.shape), tuple(gout.shape)}
    kqv_view, gout_view = as_view(kqv, kind), as_view(gout, kind)
    got, copies = recorded_copies(lambda: gpu_attention(kqv_view, gout_view, counts, 40), shapes)
    assert no_nan(got) and not copies, copies
    want = gpu_attention(fresh(kqv), fresh(gout), counts, 40)              # scalar loads only: one variant
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", [sum(VIEW_COUNTS[0]), 1])
def test_logit_loss_reads_views_through_their_leading_dimension(rows, C, mode, kind):
    gen = torch.Generator().manual_seed(70 + rows + C)
    logits = ((torch.rand(rows, C, generator=gen) - 0.5) * 100.0).to(DEV)
    targets = (SB.softmax_targets(rows, C, gen) if mode == "softmax" else torch.rand(rows, C, generator=gen) < 0.4).to(DEV)
    g = torch.tensor(2.5, device=DEV)

    def run(l):
        loss, lse, argmax, max_prob, totals = ops.logit_loss(l, targets, mode)
        grad = ops.logit_loss_backward(l, targets, mode, lse, totals, g)
        return [t for t in (loss, lse, argmax, max_prob, totals, grad) if t is not None]

    view = as_view(logits, kind)
    got, copies = recorded_copies(lambda: run(view), {tuple(logits.shape)})
    assert no_nan(t for t in got if t.is_floating_point()) and not copies, copies
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[-1]).all())
    want = run(fresh(logits))                                              # a wave per row, scalar loads: one variant
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def small_candidate_batch(counts, D, seed):
    gen = torch.Generator().manual_seed(seed)
    slots, Cn = len(counts), sum(counts)
    N = 300 if Cn > 1 else 1
    cand_slot = SB.index_of(counts, Cn > 1, seed)
    cand_idx, slot_idx = torch.randint(0, N, (Cn,), generator=gen), torch.randint(0, N, (slots,), generator=gen)
    correct = torch.tensor([-1 if k == 0 else int(torch.nonzero(cand_slot == s).flatten()[k // 2])
                            for s, k in enumerate(counts)])
    x, w = torch.randn(N, D, generator=gen), torch.randn(1, 2 * D, generator=gen) / math.sqrt(D)
    cot = torch.randn(Cn, generator=gen)
    return [t.to(DEV) for t in (x, w, cand_idx, slot_idx, cand_slot, correct, cot)]


@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("counts", VIEW_COUNTS, ids=["four_segments", "one_row"])
def test_candidate_kernel_reads_views_through_their_leading_dimension(counts, kind):
    D = 64
    x, w, cand_idx, slot_idx, cand_slot, correct, cot = small_candidate_batch(counts, D, 80 + len(counts))
    g = torch.tensor(1.75, device=DEV)

    def run(rows):
        """`rows`: x as a non-leaf (a view keeps its layout on the way into the kernel); d x arrives at `leaf`."""
        leaf = x.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        loss, scores, lse, argmax = heads.candidate_loss(rows(leaf), wl, cand_idx, slot_idx, cand_slot, correct)
        (loss * g + (scores * cot).sum()).backward()
        return {"loss": loss.detach(), "scores": scores.detach(), "lse": lse, "argmax": argmax, "d x": leaf.grad,
                "d w": wl.grad}

    got = run(lambda leaf: as_view(leaf, kind))
    assert no_nan(t for t in got.values() if t.is_floating_point())
    view, plan = as_view(x, kind), ops.build_plan([(cand_slot, cand_slot)], len(counts))
    _, copies = recorded_copies(lambda: ops.candidate_scores(view, cand_idx, slot_idx, cand_slot, plan, w, correct),
                                {tuple(x.shape)})
    assert not copies, copies                                              # the kernel itself gets the view
    if kind == "aligned":                                                  # float4 rows, as the contiguous call
        assert float4_rows(as_view(x, kind)) and all_equal(got, run(fresh))
    else:
        assert not float4_rows(as_view(x, kind))
        on_host = [host(t) for t in (x, w, cand_idx, slot_idx, cand_slot, correct, cot, g)]
        r32, r64 = SB.candidate_ref(*on_host, torch.float32), SB.candidate_ref(*on_host, torch.float64)
        for name, a, b in (("loss", r32[0], r64[0]), ("scores", r32[1], r64[1]), ("lse", r32[2], r64[2]),
                           ("d x", r32[4].grad, r64[4].grad), ("d w", r32[5].grad, r64[5].grad)):
            assert bar(got[name], a, b, name), name
