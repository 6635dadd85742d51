"""Row headers of a plan (ptgnn_amd_row_headers) and the header-first walk of the CSR aggregation.

A header record holds the first eight slot entries of a destination row, so a lane group can request them together
with the rowptr pair.  The walk folds the same slots in the same order: every output bit must be what the plain walk
gives (ops.ROW_HEADERS = False) and, for sum and max on rows up to the hub threshold, what oracle.scatter_ref gives on
the CPU.

The graph: ~400 destination rows whose in-degrees cycle through 0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 40 (nothing, part
of a header, exactly a header, a header plus clamped / full / several further groups), one row of 300 in-edges and one
of 2100 (a hub row: the hub walk owns it, the main kernel must leave it alone with or without a header).  The long-row
launch only engages with PTGNN_AMD_SIDE_MIN_EDGES=0, which is read once per process: a child process runs that case
(`python tests/test_gpu_row_headers.py long-rows`).  A second graph of ~100 rows has too few edges for a hub list: its
launches take the main kernel without the fused hub walk's leading workgroups."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

pytestmark = pytest.mark.gpu

I32 = torch.int32
DEGREES = [0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 40]
HUB_THRESHOLD = 2048


class Graph:
    """Edges in message order (type-major, shuffled inside a type) with their plan."""

    def __init__(self, num_types, rows, big):
        from ptgnn_amd import ops
        g = torch.Generator().manual_seed(100 * num_types + rows)
        deg = torch.tensor([DEGREES[i % len(DEGREES)] for i in range(rows)] + list(big))
        deg = deg[torch.randperm(deg.numel(), generator=g)]            # the long rows sit somewhere in the middle
        self.N, self.T, self.deg = int(deg.numel()), num_types, deg
        dst = torch.repeat_interleave(torch.arange(self.N), deg)
        self.E = int(dst.numel())
        order = torch.randperm(self.E, generator=g)
        dst = dst[order]
        src = torch.randint(0, self.N, (self.E,), generator=g)
        typ = torch.randint(0, num_types, (self.E,), generator=g)
        by_type = torch.argsort(typ, stable=True)
        self.src, self.dst, self.typ = src[by_type], dst[by_type], typ[by_type]
        self.adj = [(self.src[self.typ == t].cuda(), self.dst[self.typ == t].cuda()) for t in range(num_types)]
        self.plan = ops.build_plan(self.adj, self.N)
        self.small = deg <= HUB_THRESHOLD


_GRAPHS = {}


def graph(num_types, kind="hub"):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    key = (num_types, kind)
    if key not in _GRAPHS:
        _GRAPHS[key] = Graph(num_types, 400, (300, 2100)) if kind == "hub" else Graph(num_types, 100, ())
    return _GRAPHS[key]


def header_ref(rowptr, entries):
    """numpy: first eight entries of every row, clamped to the row's last slot, zeros for an empty row."""
    rowptr, entries = rowptr.cpu().numpy().astype(np.int64), entries.cpu().numpy()
    beg, end = rowptr[:-1], rowptr[1:]
    idx = np.minimum(beg[:, None] + np.arange(8)[None, :], (end - 1)[:, None])
    hdr = entries[np.clip(idx, 0, max(entries.shape[0] - 1, 0))]
    hdr[end == beg] = 0
    return hdr.astype(np.int32)


def shared_rows(g, monkeypatch):
    """UniqueMessages of the graph's plan (the small plan takes the shared-row form with the threshold at 0)."""
    from ptgnn_amd import ops
    monkeypatch.setattr(ops, "UNIQUE_MIN_EDGES", 0)
    monkeypatch.setattr(ops._device_state("cuda").uniq_backoff, "steps", 0)
    uniq = g.plan.unique_messages()
    assert uniq is not None
    return uniq


# ---------------------------------------------------------------------------------------------------------------------
# the header itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_types", [1, 5])
@pytest.mark.parametrize("kind", ["hub", "nohub"])
def test_header_is_the_first_eight_entries_of_every_row(num_types, kind, monkeypatch):
    g = graph(num_types, kind)
    plan = g.plan
    assert sorted(set(g.deg.tolist())) == sorted(set(DEGREES) | ({300, 2100} if kind == "hub" else set()))
    assert (plan.rowptr[1:] - plan.rowptr[:-1]).cpu().tolist() == g.deg.tolist()
    uniq = shared_rows(g, monkeypatch)
    for entries in (plan.col, plan.perm, uniq.slot_row):
        hdr = plan.row_header(entries)
        assert hdr.dtype == I32 and tuple(hdr.shape) == (g.N, 8) and hdr.is_contiguous() and hdr.data_ptr() % 32 == 0
        assert plan.row_header(entries) is hdr                                       # one launch per slot array
        want = header_ref(plan.rowptr, entries[: max(g.E, 1)])
        assert np.array_equal(hdr.cpu().numpy(), want)
    assert plan.row_header() is plan.row_header(plan.col) and uniq.hdr is plan.row_header(uniq.slot_row)
    assert plan.row_header(plan.perm.clone()) is None                                # a slot array the plan does not know
    # the plans that keep the plain walk carry none
    assert plan.backward_plan().row_header() is None and plan.transposed_plan().row_header() is None


# ---------------------------------------------------------------------------------------------------------------------
# the walk: same bits with and without, and the serial fold's bits
# ---------------------------------------------------------------------------------------------------------------------
def aggregate(g, form, M, reduce, uniq, header, rows=None, out=None):
    """One aggregation launch of `form` -> (out, per-slot messages in message order or None)."""
    from ptgnn_amd import ops
    gen = torch.Generator().manual_seed(M + 7 * g.T)
    ops.ROW_HEADERS = header
    kw = {} if rows is None else {"rows": rows, "out": out}
    if form == "table":                                   # per-edge form: col = (src << type_bits) | type
        y = torch.randn(g.N, g.T * M, generator=gen)
        msgs = y.view(g.N, g.T, M)[g.src, g.typ]
        res = ops.gather_reduce(y.cuda(), g.plan, M, reduce, **kw)
    elif form == "dst1":                                  # one edge type: the destination term is one row per node
        assert g.T == 1
        y, yd = torch.randn(g.N, M, generator=gen), torch.randn(g.N, M, generator=gen)
        msgs = y[g.src] + yd[g.dst]
        res = ops.gather_reduce(y.cuda(), g.plan, M, reduce, ydst=yd.cuda(), **kw)
    else:                                                 # shared rows: slot -> message row
        table = torch.randn(uniq.capacity, M, generator=gen)
        msgs = None
        res = ops.gather_reduce(table.cuda(), g.plan, M, reduce, type_bits=0, col=uniq.slot_row, **kw)
    return res, msgs


CASES = [(T, M, form) for T in (1, 5) for M in (64, 128, 256, 320) for form in ("table", "shared", "dst1")
         if not (form == "dst1" and T != 1)]


@pytest.mark.parametrize("reduce", ["sum", "max", "min", "mean"])
@pytest.mark.parametrize("num_types,M,form", CASES)
def test_outputs_have_the_same_bits_with_and_without_headers(num_types, M, form, reduce, monkeypatch):
    """Whole-matrix and row-range launches (the range starts mid-tile), widths of 16 / 32 / 64 lanes per row and one of
    two column chunks (320: no header walk, the header must not be built), every reduce, the three message forms (the
    destination-term form stays on the plain walk: no header is built for it either)."""
    from oracle import scatter_ref
    from ptgnn_amd import ops
    monkeypatch.setattr(ops, "ROW_HEADERS", True)         # restored after the test whatever `aggregate` leaves
    for kind in ("hub", "nohub"):
        g = graph(num_types, kind)
        plan = g.plan
        uniq = shared_rows(g, monkeypatch) if form == "shared" else None
        plan._hdrs.clear()
        if uniq is not None:
            uniq.hdr = None
        off, msgs = aggregate(g, form, M, reduce, uniq, header=False)
        assert not plan._hdrs and (uniq is None or uniq.hdr is None)                 # the switch is looked at per call
        on, _ = aggregate(g, form, M, reduce, uniq, header=True)
        built = (uniq.hdr is not None) if form == "shared" else ("col" in plan._hdrs)
        assert built == (M <= 256 and form != "dst1"), (M, form, built)    # built only for the kernels that read it
        assert torch.equal(on.view(I32), off.view(I32)), torch.nonzero((on != off).any(1)).flatten()[:8].tolist()
        # destination rows [lo, hi): lo is no multiple of the 4 / 8 / 16 rows of a workgroup's tile
        lo, hi = 13, g.N - 5
        for header in (True, False):
            part = torch.full((g.N, M), 7.25, device="cuda")
            aggregate(g, form, M, reduce, uniq, header, rows=(lo, hi), out=part)
            assert torch.equal(part[lo:hi].view(I32), on[lo:hi].view(I32)), header
            assert bool((part[:lo] == 7.25).all()) and bool((part[hi:] == 7.25).all()), header
        if reduce in ("sum", "max"):
            if msgs is None:                              # shared rows: the message of a slot, slots in CSR order
                table = torch.randn(uniq.capacity, M, generator=torch.Generator().manual_seed(M + 7 * g.T))
                msgs = table[uniq.slot_row[: g.E].cpu().long()]
                dst = torch.repeat_interleave(torch.arange(g.N), g.deg)
            else:
                dst = g.dst
            want = scatter_ref.scatter(msgs, dst, dim=0, dim_size=g.N, reduce=reduce)
            bad = (on.cpu().view(I32) != want.view(I32)).any(1) & g.small
            assert not bool(bad.any()), (kind, torch.nonzero(bad).flatten()[:8].tolist(), g.deg[bad][:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------------------------------------------------
def _minibatch():
    from ptgnn_amd import workloads
    mb = workloads.batched_graphs(3, 500, 8, 2.2, seed=31)
    adj = [(s.cuda(), d.cuda()) for s, d in mb["adjacency_lists"]]
    return mb, adj, mb["node_to_graph_idx"].cuda()


def _net(which):
    from benchmarks import graph2class as G2C
    from ptgnn_amd import layers as L
    from ptgnn_amd.gnn import GraphNeuralNetwork
    torch.manual_seed(5)
    if which == "layer":
        mods = [L.GatedMessagePassingLayer(128, 128, 17, "max")]
    else:
        mods = G2C.typilus_stack("ggnn", 128, 17, 0.1, agg="max")
    return GraphNeuralNetwork(mods, torch.nn.Identity(), True, True).cuda().eval()


def _forward(net, x, adj, n2g, num_graphs):
    from ptgnn_amd import ops
    ops.clear_plan_cache()
    with torch.no_grad():
        out = net(node_data={"input": x}, adjacency_lists=adj, edge_feature_data=[], node_to_graph_idx=n2g,
                  reference_node_ids={}, reference_node_graph_idx={}, num_graphs=num_graphs)
    return out.output_node_representations


def _plan_has_header():
    from ptgnn_amd import ops
    plan = ops._PLAN_CACHE[0]
    return bool(plan._hdrs) or bool(plan._uniq and plan._uniq.hdr is not None)


@pytest.mark.parametrize("shared", [False, True], ids=["per-edge", "shared-rows"])
@pytest.mark.parametrize("which", ["layer", "typilus-stack"])
def test_ggnn_layer_and_typilus_stack_give_the_same_bits_with_and_without_headers(which, shared, monkeypatch):
    from ptgnn_amd import ops, workloads
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if shared:
        monkeypatch.setattr(ops, "UNIQUE_MIN_EDGES", 0)
        monkeypatch.setattr(ops._device_state("cuda").uniq_backoff, "steps", 0)
    mb, adj, n2g = _minibatch()
    assert 1200 <= mb["num_nodes"] <= 1800
    net = _net(which)
    x = workloads.node_states(mb["num_nodes"], 128, seed=3).cuda()
    monkeypatch.setattr(ops, "ROW_HEADERS", False)
    off = _forward(net, x, adj, n2g, mb["num_graphs"])
    assert not _plan_has_header()
    monkeypatch.setattr(ops, "ROW_HEADERS", True)
    on = _forward(net, x, adj, n2g, mb["num_graphs"])
    assert _plan_has_header()
    assert shared == bool(ops._PLAN_CACHE[0]._uniq)
    assert torch.equal(on.view(I32), off.view(I32)), float((on - off).abs().max())


def test_plan_and_layer_with_headers_capture_and_replay_with_the_same_bits(monkeypatch):
    """The plan build, the header launch and the layer under stream capture; the replay on new node states gives the
    bits of the eager plain walk."""
    from ptgnn_amd import ops, workloads
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    mb, adj, n2g = _minibatch()
    net = _net("layer")
    N = mb["num_nodes"]
    x_static = workloads.node_states(N, 128, seed=1).cuda()
    monkeypatch.setattr(ops, "ROW_HEADERS", True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _forward(net, x_static, adj, n2g, mb["num_graphs"])          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        y_static = _forward(net, x_static, adj, n2g, mb["num_graphs"])
        assert _plan_has_header()                                          # built inside the capture
    x_new = workloads.node_states(N, 128, seed=2).cuda()
    x_static.copy_(x_new)
    graph_.replay()
    got = y_static.clone()
    monkeypatch.setattr(ops, "ROW_HEADERS", False)
    want = _forward(net, x_new, adj, n2g, mb["num_graphs"])
    assert torch.equal(got.view(I32), want.view(I32))


# ---------------------------------------------------------------------------------------------------------------------
# the long-row launch next to the header walk (environment read once per process: a child process)
# ---------------------------------------------------------------------------------------------------------------------
def _long_rows_child():
    """PTGNN_AMD_SIDE_MIN_EDGES=0: the row of 300 in-edges folds in k_long_rows and the hub row in k_hub_chunks, both on
    side streams, while the main kernel walks the other rows header-first."""
    from oracle import scatter_ref
    from ptgnn_amd import ops
    assert os.environ.get("PTGNN_AMD_SIDE_MIN_EDGES") == "0"
    for T, form in ((1, "table"), (5, "table")):
        g = Graph(T, 400, (300, 2100))
        for reduce in ("sum", "max"):
            off, msgs = aggregate(g, form, 128, reduce, None, header=False)
            on, _ = aggregate(g, form, 128, reduce, None, header=True)
            assert "col" in g.plan._hdrs
            assert torch.equal(on.view(I32), off.view(I32)), (T, form, reduce)
            want = scatter_ref.scatter(msgs, g.dst, dim=0, dim_size=g.N, reduce=reduce)
            bad = (on.cpu().view(I32) != want.view(I32)).any(1) & g.small
            assert not bool(bad.any()), (T, form, reduce, g.deg[bad][:8].tolist())
    print("long-rows ok")


def test_long_row_and_hub_launches_beside_the_header_walk_in_a_child():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, PTGNN_AMD_SIDE_MIN_EDGES="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "long-rows"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    tail = (r.stdout + "\n" + r.stderr)[-4000:]
    assert r.returncode == 0 and "long-rows ok" in r.stdout, tail


if __name__ == "__main__" and sys.argv[1:] == ["long-rows"]:
    _long_rows_child()
