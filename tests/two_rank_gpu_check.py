"""Worker of tests/test_gpu_two_rank.py: REAL separate processes, one per rank, all on cuda:0, process group
`gloo` (its CUDA all-to-all / all-reduce paths), so that the per-minibatch halo bookkeeping, the per-layer
all-to-all(v), the asynchronous two-block exchange, the transposed exchange of the backward and the pool
all-reduce of the global-exchange layers run over an actual rendezvous instead of the single-process
"virtual rank" stand-ins of test_gpu_parity.py.  (RCCL refuses two ranks on one device and `gpurun` boxes have
one GPU; the collectives' semantics are the backend-independent part, and that is what is checked here.)

Launch: python -m torch.distributed.run --nproc-per-node W --master-addr 127.0.0.1 --master-port P \
            tests/two_rank_gpu_check.py
Every rank computes the UNSHARDED result itself (same seeds) and compares its own row range.
Prints one line `rank R ok <case>` per passed case; exits non-zero on the first mismatch."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ranges(adj, n, world):
    from ptgnn_amd import sharded
    indeg = torch.zeros(n, dtype=torch.int64)
    for _, d in adj:
        indeg += torch.bincount(d, minlength=n)
    return sharded.balanced_node_ranges(indeg, world)


def _mine(adj, lo, hi):
    return [(s[(d >= lo) & (d < hi)].cuda(), d[(d >= lo) & (d < hi)].cuda()) for s, d in adj]


def _cuda_adj(adj):
    return [(s.cuda(), d.cuda()) for s, d in adj]


def _ok(rank, case):
    print(f"rank {rank} ok {case}", flush=True)


def case_layers(rank, world):
    """Single layers, inference: edge form (T = 17, ships node states), table form (T = 1, ships message rows),
    plain and two-block (asynchronous all-to-all) modes -- bit-identical to the unsharded layer (two-block sums:
    within 1e-6, the partials re-associate)."""
    from oracle import mp_oracle as O          # augmentation helper only (tests may use the oracle)
    from ptgnn_amd import layers as L, ops, sharded, workloads
    H = 64
    mb = workloads.batched_graphs(6, 700, 8, 2.2, seed=31)
    n = mb["num_nodes"]
    adj17 = O.augment_adjacency(mb["adjacency_lists"], n, True, True)
    g = torch.Generator().manual_seed(17)
    adj1 = [(torch.randint(0, n, (5 * n,), generator=g), torch.randint(0, n, (5 * n,), generator=g))]
    x = workloads.node_states(n, H, seed=32).cuda()
    for name, adj, make in (
            ("ggnn_edge_max", adj17, lambda T: L.GatedMessagePassingLayer(H, H, T, "max")),
            ("mlp_edge_sum", adj17, lambda T: L.MlpMessagePassingLayer(H, H, H, T, "sum")),
            ("mlp_table_sum", adj1, lambda T: L.MlpMessagePassingLayer(H, H, H, T, "sum")),
            ("ggnn_table_min", adj1, lambda T: L.GatedMessagePassingLayer(H, H, T, "min"))):
        # pin the form: a shard and the whole graph must not land on different sides of the edge / table choice
        L.EDGE_PATH_BIAS = 0.0 if adj is adj17 else 1e9
        torch.manual_seed(33)
        layer = make(len(adj)).cuda().eval()
        cadj = _cuda_adj(adj)
        ops.clear_plan_cache()
        with torch.no_grad():
            want = layer(x, cadj, None, {}, {}, [None] * len(cadj))
        ranges = _ranges(adj, n, world)
        lo, hi = ranges[rank]
        for overlap in (False, True):
            shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi), overlap=overlap,
                                               all_ranges=None if overlap else ranges)
            assert shard.n_halo > 0 and not shard.no_cut
            with torch.no_grad():
                got = layer.forward_sharded(x[lo:hi].contiguous(), shard)
            if overlap and name.endswith("sum"):
                # two-block mode: (own partial) + (halo partial) instead of the CSR fold order (sharded.py)
                err = float((got - want[lo:hi]).abs().max())
                assert err <= 1e-6 * max(1.0, float(want.abs().max())), err
            else:
                np.testing.assert_array_equal(got.cpu().numpy(), want[lo:hi].cpu().numpy())
            _ok(rank, f"{name}{'_two_block' if overlap else ''}")


def case_stack(rank, world):
    """varmisuse/train.py:76-107 through sharded.run_stack with graphs that STRADDLE the rank boundaries: the
    per-graph pools are combined across ranks (all-reduce), which re-associates the fp32 sums: <= 1e-5."""
    from oracle import mp_oracle as O
    from ptgnn_amd import layers as L, ops, reduceops as R, sharded, workloads
    from ptgnn_amd.gnn import GraphNeuralNetwork
    H = 64
    L.EDGE_PATH_BIAS = 1.25                      # the shipped default (earlier cases pinned it)
    mb = workloads.batched_graphs(5, 900, 4, 2.2, seed=41)
    n, n2g = mb["num_nodes"], mb["node_to_graph_idx"]
    adj = O.augment_adjacency(mb["adjacency_lists"], n, True, True)
    T = len(adj)
    torch.manual_seed(42)
    ggnn = L.GatedMessagePassingLayer(H, H, T, "sum")
    r1, r2 = L.MeanResidualLayer(H), L.MeanResidualLayer(H)
    g1 = R.GruGlobalStateUpdate(R.WeightedSumVarSizedElementReduce(H), H, H)
    g2 = R.GruGlobalStateUpdate(R.SimpleVarSizedElementReduce("max"), H, H)
    mods = [r1.pass_through_dummy_layer(), r2.pass_through_dummy_layer(), ggnn, ggnn, g1, ggnn, r1,
            ggnn, g2, ggnn, r2]
    net = GraphNeuralNetwork(mods, torch.nn.Identity(), True, True).cuda().eval()
    x = workloads.node_states(n, H, seed=43).cuda()
    ops.clear_plan_cache()
    with torch.no_grad():
        want = net(node_data={"input": x}, adjacency_lists=_cuda_adj(mb["adjacency_lists"]), edge_feature_data=[],
                   node_to_graph_idx=n2g.cuda(), reference_node_ids={}, reference_node_graph_idx={},
                   num_graphs=mb["num_graphs"]).output_node_representations
    ranges = _ranges(adj, n, world)
    lo, hi = ranges[rank]
    assert int(n2g[lo]) == int(n2g[lo - 1]) if rank > 0 else True          # the cut is inside a graph
    shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi))
    shard.attach_graph_index(n2g[lo:hi].cuda(), mb["num_graphs"])
    with torch.no_grad():
        got = sharded.run_stack(mods, x[lo:hi].contiguous(), shard)
    err = float((got - want[lo:hi]).abs().max())
    assert err <= 1e-5, err
    _ok(rank, f"ggnn_stack_global_exchange err={err:.2e}")


def case_training(rank, world):
    """One training step over the shard (edge form and table form): loss = sum over ranks of <y_local, g_local>;
    parameter gradients summed over ranks (what DDP does) and the input gradient of the own rows must equal the
    whole-graph step's (fp32 re-association only: 2e-5 x scale, the tolerance of the single-GPU gradient tests)."""
    from oracle import mp_oracle as O
    from ptgnn_amd import layers as L, ops, sharded, workloads
    H = 64
    mb = workloads.batched_graphs(4, 600, 6, 2.2, seed=51)
    n = mb["num_nodes"]
    adj13 = O.augment_adjacency(mb["adjacency_lists"], n, True, True)
    g = torch.Generator().manual_seed(52)
    adj1 = [(torch.randint(0, n, (4 * n,), generator=g), torch.randint(0, n, (4 * n,), generator=g))]
    x = workloads.node_states(n, H, seed=53).cuda()
    gout = torch.randn(n, H, generator=g).cuda()
    for name, adj, make in (
            ("train_ggnn_edge_max", adj13, lambda T: L.GatedMessagePassingLayer(H, H, T, "max")),
            ("train_mlp_table_sum", adj1, lambda T: L.MlpMessagePassingLayer(H, H, H, T, "sum"))):
        L.EDGE_PATH_BIAS = 0.0 if adj is adj13 else 1e9
        torch.manual_seed(54)
        layer = make(len(adj)).cuda().train()
        cadj = _cuda_adj(adj)
        layer.zero_grad()
        xi = x.clone().requires_grad_(True)
        ops.clear_plan_cache()
        y = layer(xi, cadj, None, {}, {}, [None] * len(cadj))
        y.backward(gout)
        want = [y.detach(), xi.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        ranges = _ranges(adj, n, world)
        lo, hi = ranges[rank]
        layer.zero_grad()
        shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi), all_ranges=ranges)
        xl = x[lo:hi].clone().requires_grad_(True)
        yl = layer.forward_sharded(xl, shard)
        yl.backward(gout[lo:hi])
        got_p = []
        for p in layer.parameters():
            gp = p.grad.clone() if p.grad is not None else torch.zeros_like(p)
            dist.all_reduce(gp)
            got_p.append(gp)
        pairs = [(yl.detach(), want[0][lo:hi]), (xl.grad, want[1][lo:hi])] + list(zip(got_p, want[2:]))
        worst = 0.0
        for a, b in pairs:
            sc = max(1.0, float(b.abs().max()))
            worst = max(worst, float((a - b).abs().max()) / sc)
        assert worst <= 2e-5, worst
        _ok(rank, f"{name} rel_err={worst:.2e}")


def case_graph_boundaries(rank, world):
    """The cfg4-shaped stack over a partition SNAPPED TO GRAPH STARTS (sharded.ranges_on_graph_boundaries): the
    build finds no cut edge (one all-reduce), `assume_no_cut=True` skips even that (no collective, no read-back),
    and both give the unsharded rows bit for bit -- no halo, no exchange, the single-GPU kernels per rank."""
    from oracle import mp_oracle as O
    from ptgnn_amd import layers as L, ops, sharded, workloads
    H = 64
    L.EDGE_PATH_BIAS = 1.25
    mb = workloads.batched_graphs(9, 500, 5, 2.4, seed=61)
    n, n2g = mb["num_nodes"], mb["node_to_graph_idx"]
    adj = O.augment_adjacency(mb["adjacency_lists"], n, True, True)
    T = len(adj)
    torch.manual_seed(62)
    r1 = L.ConcatResidualLayer(H)
    mods = [r1.pass_through_dummy_layer(), L.MlpMessagePassingLayer(H, H, H, T, "max"),
            L.MlpMessagePassingLayer(H, H, H, T, "max"), r1, L.MlpMessagePassingLayer(2 * H, H, 2 * H, T, "max")]
    mods = [m.cuda().eval() for m in mods]
    x = workloads.node_states(n, H, seed=63).cuda()
    cadj = _cuda_adj(adj)
    ops.clear_plan_cache()
    with torch.no_grad(), L.forward_scope():
        want = x
        for m in mods:
            want = m(want, cadj, n2g.cuda(), {}, {}, [None] * T)
    indeg = torch.zeros(n, dtype=torch.int64)
    for _, d in adj:
        indeg += torch.bincount(d, minlength=n)
    ranges = sharded.ranges_on_graph_boundaries(n2g, indeg, world)
    lo, hi = ranges[rank]
    for assume in (False, True):
        shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi), all_ranges=ranges, assume_no_cut=assume)
        assert shard.no_cut and shard.n_halo == 0
        shard.attach_graph_index(n2g[lo:hi].cuda(), mb["num_graphs"])
        with torch.no_grad():
            got = sharded.run_stack(mods, x[lo:hi].contiguous(), shard)
        np.testing.assert_array_equal(got.cpu().numpy(), want[lo:hi].cpu().numpy())
        _ok(rank, f"graph_boundary_partition{'_assumed' if assume else '_detected'}")
    ops.check_indices(sync=True)     # the range guard saw no source outside the own rows


def case_planner(rank, world):
    """Learned exchange capacities on the DEVICE path (HIP index pass, HIP row gather, torch remap): three cut-edge
    minibatches of different sizes through ONE ExchangePlanner -- the first build is exact, the next two make no blocking
    host read (sharded.HOST_READS) -- each bit-identical to the unsharded layer (max: any fold order; padding rows of the
    halo table are never referenced)."""
    from ptgnn_amd import layers as L, ops, sharded, workloads
    H = 64
    L.EDGE_PATH_BIAS = 1e9                         # table form: message rows travel
    torch.manual_seed(81)
    layer = L.MlpMessagePassingLayer(H, H, H, 1, "max").cuda().eval()
    planner = sharded.ExchangePlanner()
    n = 6000
    ranges = [(p * n // world, (p + 1) * n // world) for p in range(world)]
    lo, hi = ranges[rank]
    for i, e in enumerate((30_000, 24_000, 27_000)):
        g = torch.Generator().manual_seed(82 + i)
        adj = [(torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g))]
        x = workloads.node_states(n, H, seed=90 + i).cuda()
        ops.clear_plan_cache()
        with torch.no_grad():
            want = layer(x, _cuda_adj(adj), None, {}, {}, [None])[lo:hi]
        before = dict(sharded.HOST_READS)
        shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi), all_ranges=ranges, planner=planner)
        with torch.no_grad():
            got = layer.forward_sharded(x[lo:hi].contiguous(), shard)
        blocking = sharded.HOST_READS["blocking"] - before["blocking"]
        assert blocking == (1 if i == 0 else 0), (i, blocking)
        assert not shard.no_cut and shard.n_halo > 0
        if i:       # steady state: the halo table holds every pair's learned capacity (the exact first build: the true counts)
            assert shard.n_halo == sum(planner.recv_caps) == sum(shard.recv_splits)
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    assert planner.exact_builds == 1 and planner.builds == 3 and planner.overflows == 0
    ops.check_indices(sync=True)
    _ok(rank, f"planner_steady_state halo_capacity={sum(planner.recv_caps)}")


def case_fuzz(rank, world):
    """Seeded random sweep over real collectives: random graphs (1-5 edge types, some empty, a hot destination), widths,
    reduces, layer kinds and forms; every build goes through ONE ExchangePlanner shared by all cases, so later (larger)
    graphs overflow the capacities learned from earlier ones -- the next build then raises on EVERY rank, is repeated, and
    the truncated minibatch is recomputed.  Own rows must equal the unsharded layer bit for bit (max / min always; sums too:
    a row is reduced on one rank in the unsharded order; no row here reaches the hub threshold)."""
    from ptgnn_amd import layers as L, ops, sharded
    from ptgnn_amd._lib import PtgnnAmdError
    planner = sharded.ExchangePlanner()
    raised = 0
    rng = np.random.RandomState(4242)            # the SAME stream on every rank
    for case in range(10):
        n = (600, 600, 2500, 9000, 2500, 9000, 600, 9000, 2500, 9000)[case]      # growing: capacities learned small overflow
        T = int(rng.choice([1, 2, 5]))
        H = int(rng.choice([32, 64, 128]))
        kind = ["ggnn", "mlp", "mlp_notarget"][rng.randint(3)]
        agg = ["sum", "mean", "max", "min"][rng.randint(4)]
        L.EDGE_PATH_BIAS = 0.0 if (T > 1 and rng.rand() < 0.5) else 1e9       # pin the form (shard and whole graph alike)
        adj = []
        for t in range(T):
            e = 0 if (T > 1 and rng.rand() < 0.2) else int(rng.randint(n, 6 * n))
            s_, d_ = rng.randint(0, n, e), rng.randint(0, n, e)
            if e > 100:
                d_[:300] = rng.randint(0, n)                                   # a hot destination (< hub threshold)
            adj.append((torch.from_numpy(s_.astype(np.int64)), torch.from_numpy(d_.astype(np.int64))))
        if sum(int(a[0].shape[0]) for a in adj) == 0:
            continue
        torch.manual_seed(100 + case)
        layer = (L.GatedMessagePassingLayer(H, H, T, agg) if kind == "ggnn" else
                 L.MlpMessagePassingLayer(H, H, H, T, agg, use_target_state_as_message_input=kind == "mlp")).cuda().eval()
        x = torch.randn(n, H, generator=torch.Generator().manual_seed(200 + case)).cuda()
        cadj = _cuda_adj(adj)
        ops.clear_plan_cache()
        with torch.no_grad():
            want = layer(x, cadj, None, {}, {}, [None] * T)
        ranges = _ranges(adj, n, world)
        lo, hi = ranges[rank]
        mine = _mine(adj, lo, hi)

        def run():
            shard = sharded.ShardedGraph.build(mine, (lo, hi), all_ranges=ranges, planner=planner)
            with torch.no_grad():
                return layer.forward_sharded(x[lo:hi].contiguous(), shard)
        try:
            got = run()
        except PtgnnAmdError as exc:              # the PREVIOUS case overflowed: every rank is here together
            assert "learned capacity" in str(exc)
            raised += 1
            got = run()
        # did THIS build overflow?  its count is known one build late: look now (a blocking look is fine in a test)
        pending = planner._pending
        over = pending.values(wait=True)[4] if pending is not None else 0
        if over:
            try:
                got = run()                         # raises (capacities grown) ...
                raise AssertionError("an overflow went unreported")
            except PtgnnAmdError:
                raised += 1
                got = run()                         # ... and the repeat is exact
        np.testing.assert_array_equal(got.cpu().numpy(), want[lo:hi].cpu().numpy())
    L.EDGE_PATH_BIAS = 1.25
    total = torch.tensor([raised])
    dist.all_reduce(total)
    assert int(total) == raised * world and raised >= 2   # every rank raised the same number of times
    _ok(rank, f"fuzz_planner_real_collectives overflows_recovered={raised} exact_builds={planner.exact_builds} builds={planner.builds}")


def case_powerlaw_hubs(rank, world):
    """BASELINE config 5's shape, scaled: ONE power-law graph (Zipf-0.8 destinations => hub rows of > 2048 in-edges,
    long rows of 257..2048) whose sources are uniform over ALL ranks' nodes, so every hub row has in-edges from every
    rank and (world - 1) / world of the edges are cut; one GGNN layer (T = 1: table form, message rows travel) and one
    MLP-MP layer, H = 64.  max is bit-identical to the unsharded layer on every row; a sum is bit-identical on ordinary
    rows; on hub rows the GRU output is within 1e-4 (a hub row folds chunk-wise, a shard's chunk boundaries sit
    elsewhere, and fp32 is not 1e-5-accurate for such sums in any order: DESIGN.md section 6)."""
    from ptgnn_amd import layers as L, ops, sharded, workloads
    H, n, E = 64, 160_000, 1_600_000
    adj = workloads.power_law_graph(n, E, alpha=0.8, seed=71)
    g = torch.Generator().manual_seed(72)
    adj = [(torch.randint(0, n, (E,), generator=g), adj[0][1])]        # sources uniform over every rank's range
    indeg = torch.bincount(adj[0][1], minlength=n)
    assert int(indeg.max()) > ops.HUB_THRESHOLD
    x = workloads.node_states(n, H, seed=73).cuda()
    L.EDGE_PATH_BIAS = 1.25
    ranges = _ranges(adj, n, world)
    lo, hi = ranges[rank]
    hubs = (indeg[lo:hi] > ops.HUB_THRESHOLD).cuda()
    cadj = _cuda_adj(adj)
    src_owner = torch.bucketize(adj[0][0], torch.tensor([r[1] for r in ranges]), right=True)
    for name, make in (("ggnn_sum", lambda: L.GatedMessagePassingLayer(H, H, 1, "sum")),
                       ("ggnn_max", lambda: L.GatedMessagePassingLayer(H, H, 1, "max")),
                       ("mlp_max", lambda: L.MlpMessagePassingLayer(H, H, H, 1, "max"))):
        torch.manual_seed(74)
        layer = make().cuda().eval()
        ops.clear_plan_cache()
        with torch.no_grad():
            want = layer(x, cadj, None, {}, {}, [None])[lo:hi]
        shard = sharded.ShardedGraph.build(_mine(adj, lo, hi), (lo, hi), all_ranges=ranges)
        assert not shard.no_cut and shard.n_halo > 0
        if bool(hubs.any()):      # the largest hub of this rank has sources on every rank
            hub = lo + int(torch.argmax(indeg[lo:hi]))
            assert len(torch.unique(src_owner[adj[0][1] == hub])) == world
        with torch.no_grad():
            got = layer.forward_sharded(x[lo:hi].contiguous(), shard)
        if name.endswith("max"):
            np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
        else:
            assert torch.equal(got[~hubs], want[~hubs])
            if bool(hubs.any()):
                # an un-normalised fp32 sum of 10^3..10^5 messages feeding a GRU: two legitimate fold orders differ by
                # more than 1e-5 (the fp32 oracle itself sits ~2e-4 from float64 on such rows)
                err = float((got[hubs] - want[hubs]).abs().max())
                assert err <= 1e-4, err
        _ok(rank, f"powerlaw_{name} hubs_here={int(hubs.sum())} halo={shard.n_halo}")


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    which = os.environ.get("TWO_RANK_CASES", "default")
    cases = {"default": (case_layers, case_stack, case_training, case_graph_boundaries, case_planner, case_fuzz),
             "powerlaw": (case_powerlaw_hubs,)}[which]
    try:
        for case in cases:
            case(rank, world)
            dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
