"""Destination-range sharding of ONE large batched graph across the GPUs of a node
(BASELINE.json north_star).  The reference has no counterpart: its only multi-GPU
mode is whole-batch data parallelism (ptgnn/baseneuralmodel/distributedtrainer.py:250-297), which on
ROCm runs unchanged over RCCL.  This module is the new exchange step the north star asks for.

Layout, one process per GPU:
  * rank p owns the contiguous node range [lo_p, hi_p) and ALL in-edges of those nodes (so every
    destination row is reduced on exactly one GPU, in the single-GPU message order => results equal
    the unsharded kernel's);
  * per minibatch (plan time) every rank de-duplicates the remote source ids it needs per peer and
    tells each peer which of ITS rows to send (two small all-to-alls of counts and ids);
  * per layer ONE all-to-all(v) of halo rows (RCCL over xGMI: a dedicated link per peer pair, so an
    all-to-all uses all 7 links at once, unlike a ring).  The rows exchanged are the
    message-table rows when that is no wider than the state (T*M <= H, e.g. T = 1), else the node
    states, which are then pre-transformed locally (weights are replicated).
  * local table = [own rows | halo rows from peer 0 | halo rows from peer 1 | ...]; edge sources are
    remapped into that table once per minibatch and one dst-sorted plan is built over it.

The index bookkeeping and the exchange are device-agnostic `torch`/`torch.distributed` plumbing
(they also run under gloo on CPU, which is how tests/test_sharded_cpu.py covers the N > 1 logic);
the compute stays in the HIP kernels and refuses CPU tensors.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import os

import torch
import torch.distributed as dist

from ptgnn_amd import ops
from ptgnn_amd._readback import Readback

Adj = List[Tuple[torch.Tensor, torch.Tensor]]


def _flatten(adjacency_lists: Adj):
    """The T per-type lists as ONE (src, dst) pair + the per-type edge counts (host ints, from the shapes).  All
    the per-minibatch bookkeeping below runs once over the concatenation -- a program graph has T ~ 20 edge types
    and a per-type loop of tiny torch kernels costs more than the layers it prepares (cfg4: 1.8 ms of launches
    against a 1.6 ms forward)."""
    counts = [int(s_.shape[0]) for s_, _ in adjacency_lists]
    if len(adjacency_lists) == 1:
        return adjacency_lists[0][0], adjacency_lists[0][1], counts
    return (torch.cat([s_ for s_, _ in adjacency_lists]), torch.cat([d_ for _, d_ in adjacency_lists]), counts)


def _unflatten(src: torch.Tensor, dst: torch.Tensor, counts: Sequence[int]) -> Adj:
    """Per-type views (contiguous slices) of a concatenated pair."""
    return list(zip(src.split(list(counts)), dst.split(list(counts))))


def _to_device_ints(values: Sequence[int], device) -> torch.Tensor:
    """Small host list -> device int64 without stalling the stream (pinned staging for CUDA)."""
    t = torch.tensor(list(values), dtype=torch.int64)
    if torch.device(device).type == "cuda":
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


# Device -> host reads made by the shard builds.  "blocking": the host waits for work it has just enqueued (a `.tolist()`
# of this minibatch's counts: the stream drains first); "late": values of the PREVIOUS minibatch, copied asynchronously
# when that minibatch was built and picked up now (the copy finished long ago: the host does not wait).  The steady state
# of a build with an `ExchangePlanner` makes no blocking read (tests/test_sharded_cpu.py, tests/two_rank_gpu_check.py).
HOST_READS = {"blocking": 0, "late": 0}


def _read_now(t: torch.Tensor) -> list:
    HOST_READS["blocking"] += 1
    return t.tolist()


class ExchangePlanner:
    """Learned capacities of the per-layer halo exchange, kept ACROSS the minibatches of one process group (one planner
    per model / data loader and rank; every rank of the group must use one).

    `ShardedGraph.build` needs host integers for the all-to-all of halo rows: how many rows travel per peer pair.  The
    exact build reads them back from the device once per minibatch -- a blocking read that drains the stream, of the same
    order as a whole cfg4 forward.  With a planner only the FIRST build (and a build after an overflow) does that.  Every
    later build exchanges FIXED-capacity blocks instead: per peer pair the largest count seen so far x `slack`, rounded up
    to `granule` rows (grow-only; both ends of a pair learn from the same number, need_counts[p <- q] == got_counts[q -> p],
    by the same rule at the same build, so their split sizes always agree).  Unused capacity is padding: requests for the
    owner's first row, never referenced by an edge.  The true counts of build k are copied to the host asynchronously and
    looked at during build k + 1: if a pair exceeded its capacity (summed over the group, so every rank sees it), that
    build raises PtgnnAmdError on EVERY rank -- the outputs of minibatch k were computed from a truncated halo and are
    wrong (the same contract as the asynchronous node-id guard, ptgnn_amd.ops.check_indices) -- with the capacities
    already grown, so repeating the build succeeds.  `last_overflow` keeps the count for callers that prefer to poll."""

    def __init__(self, slack: float = 1.125, granule: int = 64):
        self.slack, self.granule = float(slack), int(granule)
        self.recv_caps: Optional[List[int]] = None      # rows reserved per owner in this rank's halo table
        self.send_caps: Optional[List[int]] = None      # rows this rank sends per peer
        self.global_stats: Tuple[int, int, int] = (0, 0, 0)
        self.ever_cut = False
        self._pending: Optional[Readback] = None          # the previous build's counts, on their way to the host
        self._layout = None                               # device tensors derived from the capacities (rebuilt on growth)
        self.builds = self.exact_builds = self.overflows = 0
        self.last_overflow = 0

    def ready(self) -> bool:
        return self.recv_caps is not None

    def _cap(self, old: int, seen: int) -> int:
        if seen <= old:
            return old
        want = int(seen * self.slack + 0.999)
        return (want + self.granule - 1) // self.granule * self.granule

    def learn(self, need: Sequence[int], got: Sequence[int], stats: Sequence[int]) -> None:
        old_r = self.recv_caps or [0] * len(need)
        old_s = self.send_caps or [0] * len(got)
        new_r = [self._cap(o, int(c)) for o, c in zip(old_r, need)]
        new_s = [self._cap(o, int(c)) for o, c in zip(old_s, got)]
        if new_r != self.recv_caps or new_s != self.send_caps:
            self._layout = None
        self.recv_caps, self.send_caps = new_r, new_s
        self.global_stats = (int(stats[1]), int(stats[2]), int(stats[3]))
        self.ever_cut = self.ever_cut or int(stats[0]) > 0

    def post(self, values: torch.Tensor) -> None:
        """Start the asynchronous copy of this build's counts to the host (read by the next build; CPU counts, as under
        gloo, are there at once)."""
        self._pending = Readback(values)

    def collect(self, world: int) -> None:
        """Look at the previous build's counts (posted one minibatch ago): learn from them; an overflow raises."""
        pending, self._pending = self._pending, None
        if pending is None:
            return
        vals = pending.values(wait=True)    # posted a whole minibatch ago: already there, the host does not wait
        HOST_READS["late"] += 1
        stats, need, got = vals[:5], vals[5: 5 + world], vals[5 + world: 5 + 2 * world]
        self.learn(need, got, stats)
        self.last_overflow = stats[4]
        if stats[4] > 0:
            self.overflows += 1
            from ptgnn_amd import _lib
            raise _lib.PtgnnAmdError(
                f"halo exchange: {stats[4]} (rank, owner) pair(s) needed more halo rows than the learned capacity in the "
                "PREVIOUS sharded minibatch; its halo table was truncated and its outputs are wrong.  The capacities "
                "have been grown: rebuild (and recompute that minibatch if its results matter).")

    def layout(self, world: int, device, bounds: torch.Tensor):
        """(owner of every padded halo position, start of every owner's block, capacities) as device tensors."""
        if self._layout is None or self._layout[0].device != torch.device(device):
            caps = torch.tensor(self.recv_caps, dtype=torch.int64)
            off = torch.cumsum(caps, 0) - caps
            owner = torch.repeat_interleave(torch.arange(world, dtype=torch.int64), caps)
            if torch.device(device).type == "cuda":
                caps, off, owner = (t.pin_memory().to(device, non_blocking=True) for t in (caps, off, owner))
            self._layout = (owner, off, caps)
        return self._layout


def balanced_node_ranges(in_degree: torch.Tensor, world: int) -> List[Tuple[int, int]]:
    """Contiguous ranges with ~equal numbers of in-edges (+1 per node so empty rows count a bit):
    the balance criterion that matters for power-law graphs."""
    w = in_degree.to(torch.float64) + 1.0
    c = torch.cumsum(w, 0)
    total = float(c[-1]) if c.numel() else 0.0
    cuts = [0]
    for p in range(1, world):
        cuts.append(int(torch.searchsorted(c, torch.tensor(total * p / world, dtype=c.dtype))))
    cuts.append(int(in_degree.shape[0]))
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return [(cuts[i], cuts[i + 1]) for i in range(world)]


def ranges_on_graph_boundaries(node_to_graph_idx: torch.Tensor, in_degree: torch.Tensor, world: int
                               ) -> List[Tuple[int, int]]:
    """Contiguous node ranges with ~equal in-edge mass whose cuts are SNAPPED TO GRAPH STARTS ("choose
    boundaries on graph boundaries via node_to_graph_idx when possible").  A ptgnn minibatch is a disjoint union whose
    graphs occupy contiguous id ranges (graphneuralnetwork.py:418-423, 440-443), so such a partition cuts no edge: the
    per-layer halo exchange and its bookkeeping disappear (`ShardedGraph.build(..., assume_no_cut=True)`).  Every cut
    goes to the graph start nearest (in mass) to the ideal split point; with fewer graphs than ranks the surplus
    ranks get empty ranges.  `node_to_graph_idx` must be non-decreasing (the batcher's layout)."""
    n = int(node_to_graph_idx.shape[0])
    if n == 0:
        return [(0, 0)] * world
    g = node_to_graph_idx.to(torch.int64).cpu()
    if bool((g[1:] < g[:-1]).any()):
        raise ValueError("ranges_on_graph_boundaries: node_to_graph_idx must be sorted (graphs contiguous)")
    w = (in_degree.to(torch.float64).cpu() + 1.0)
    c = torch.cumsum(w, 0)
    total = float(c[-1])
    first = torch.ones(n, dtype=torch.bool)
    first[1:] = g[1:] != g[:-1]
    starts = torch.nonzero(first).flatten()                    # node id where each graph starts
    mass_before = torch.cat([torch.zeros(1, dtype=torch.float64), c])[starts]   # edge mass in front of each graph
    cuts = [0]
    for p in range(1, world):
        j = int(torch.argmin((mass_before - total * p / world).abs()))
        cuts.append(max(int(starts[j]), cuts[-1]))
    cuts.append(n)
    return [(cuts[i], cuts[i + 1]) for i in range(world)]


class ShardedGraph:
    """Per-rank view of a dst-range-sharded minibatch."""

    def __init__(self):
        self.rank = self.world = 0
        self.lo = self.hi = 0
        self.n_local = self.n_halo = 0
        self.bounds: Optional[torch.Tensor] = None       # int64 [world + 1] on device
        self.bounds_host: List[int] = []
        self.need_ids: Optional[torch.Tensor] = None      # global ids of halo rows, sorted
        self.send_ids: Optional[torch.Tensor] = None      # local row ids to send, grouped by peer
        self.send_splits: List[int] = []
        self.recv_splits: List[int] = []
        self.local_adj: Adj = []
        self._plan: Optional["ops.GraphPlan"] = None
        self.group = None
        self.no_cut = False    # True when NO rank has a remote source: the exchange is skipped entirely
        # sums over ALL ranks of (edges, own rows, halo rows): what the layers' edge-form / table-form choice is made
        # from.  The form fixes WHAT travels in the halo all-to-all (node states or message-table rows), so it must
        # be one decision for the whole group, not one per rank from its own shard sizes
        self.global_stats: Tuple[int, int, int] = (0, 0, 0)
        # global-exchange layers (globalgraphexchange.py): graph id of every OWN node (global graph ids) and the
        # number of graphs of the whole batch; set by the caller (`attach_graph_index`)
        self.node_to_graph_idx: Optional[torch.Tensor] = None
        self.num_graphs: int = 0
        # two-block mode (`overlap=True`): edges split by where their SOURCE lives, so the own-source block can be
        # aggregated while the halo all-to-all is in flight (SURVEY.md 8e "two CSR blocks")
        self.overlap = False
        self.adj_own: Adj = []
        self.adj_halo: Adj = []
        self.plan_own: Optional["ops.GraphPlan"] = None
        self.plan_halo: Optional["ops.GraphPlan"] = None
        self.plan_comb: Optional["ops.GraphPlan"] = None
        self._flat = self._local_flat = None             # concatenated edge list (global ids / local table ids)

    # -- construction ---------------------------------------------------------------------------
    @staticmethod
    def build(adjacency_lists: Adj, node_range: Tuple[int, int], group=None,
              build_plan: bool = True, all_ranges: Optional[Sequence[Tuple[int, int]]] = None,
              overlap: Optional[bool] = None, assume_no_cut: bool = False,
              planner: Optional["ExchangePlanner"] = None) -> "ShardedGraph":
        """adjacency_lists: int64 (src, dst) per edge type in GLOBAL node ids, holding exactly the
        edges whose dst lies in this rank's `node_range`.  `all_ranges` (every rank's range, in rank
        order) skips the all-gather when the partition is static.  `overlap` (default: env
        PTGNN_AMD_SHARD_OVERLAP, off): split the edges into an own-source and a halo-source block so that
        inference layers aggregate the first while the halo rows travel (see `aggregate_two_blocks`).
        `planner` (an `ExchangePlanner` kept across minibatches): after its first build the exchange sizes come from
        learned capacities and the build makes NO blocking host read (single-block mode; `overlap` builds stay exact)."""
        g = ShardedGraph()
        g.group = group
        if overlap is None:
            overlap = os.environ.get("PTGNN_AMD_SHARD_OVERLAP", "0") not in ("", "0")
        g.rank, g.world = dist.get_rank(group), dist.get_world_size(group)
        g.lo, g.hi = int(node_range[0]), int(node_range[1])
        g.n_local = g.hi - g.lo
        dev = adjacency_lists[0][0].device
        if assume_no_cut:
            # The caller partitioned on graph boundaries (`ranges_on_graph_boundaries`): no edge crosses a rank, so
            # there is nothing to detect, exchange or read back -- no collective, no host synchronisation, no pass
            # over the global id space; the plan build's range guard still flags a source outside the own rows
            # (ptgnn_amd.ops.check_indices), i.e. a broken promise cannot go unnoticed.  EVERY rank must pass it.
            if all_ranges is not None:
                g.set_bounds(all_ranges, dev)
            g.no_cut = True
            g.n_halo = 0
            g.need_ids = torch.zeros(0, dtype=torch.int64, device=dev)
            g.send_ids = g.need_ids
            g.send_splits = [0] * g.world
            g.recv_splits = [0] * g.world
            if g.lo == 0:
                g.local_adj = [(s_, d_) for s_, d_ in adjacency_lists]
            else:            # two launches over the concatenated lists instead of two per edge type
                src, dst, counts = _flatten(adjacency_lists)
                g.local_adj = _unflatten(src - g.lo, dst - g.lo, counts)
            g.global_stats = (0, 0, 0)      # no exchange: the form may differ per rank without harm
            g._flat = g._slot = g._mark = None
            if build_plan:
                g.build_plan()
            return g
        if all_ranges is None:   # every rank learns all range boundaries
            mine = _to_device_ints([g.lo, g.hi], dev)
            allr = [torch.empty_like(mine) for _ in range(g.world)]
            dist.all_gather(allr, mine, group=group)
            all_ranges = _read_now(torch.stack(allr))
        g.set_bounds(all_ranges, dev)

        # One tiny collective decides whether this minibatch has ANY cut edge.  A disjoint-union batch
        # partitioned on graph boundaries (graphneuralnetwork.py:418-423 keeps a graph's node ids
        # contiguous) has none: every rank then runs the single-GPU path with no data-path collective
        # and skips the halo bookkeeping altogether.
        steady = planner is not None and planner.ready() and not overlap
        if planner is not None:
            planner.builds += 1
            if steady:
                planner.collect(g.world)      # the previous minibatch's counts; an overflow raises on every rank
        ls, ld, counts, need_buf, need_counts, flag, halo_total, own_counts_dev = g._index_pass(adjacency_lists, overlap)
        n_edges = sum(counts)
        over = torch.zeros(1, dtype=torch.int64, device=dev)
        if steady:
            over = (need_counts > planner.layout(g.world, dev, g.bounds)[2]).sum().reshape(1)
        # ONE small all-reduce: the cut flag, the group-wide (edges, own rows, halo rows) the layers choose their form
        # from -- a per-rank choice would make ranks disagree on what the halo all-to-all carries -- and (planner) the
        # number of peer pairs over their learned capacity
        stats = torch.cat([flag, _to_device_ints([n_edges, g.n_local], dev), halo_total, over])
        dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
        got_counts = torch.empty_like(need_counts)
        dist.all_to_all_single(got_counts, need_counts.contiguous(), group=group)
        if steady:
            # no host read-back: fixed-capacity exchange blocks, the true counts travel to the host behind our back
            planner.post(torch.cat([stats, need_counts, got_counts]))
            g._finish_steady(planner, ls, ld, counts, need_buf, need_counts, group)
            if build_plan:
                g.build_plan()
            return g
        # ONE host read-back per minibatch: the flag + stats, the split sizes all_to_all_single wants as host ints
        # and (two-block mode) the per-type own-source edge counts
        extra = [own_counts_dev] if overlap else []
        both = _read_now(torch.cat([stats, need_counts, got_counts] + extra))
        g.global_stats = (int(both[1]), int(both[2]), int(both[3]))
        if planner is not None:
            planner.exact_builds += 1
            planner.learn(both[5: 5 + g.world], both[5 + g.world: 5 + 2 * g.world], both[:5])
        both = [both[0]] + both[5:]
        if int(both[0]) == 0:
            g.no_cut = True
            g.n_halo = 0
            g.need_ids = torch.zeros(0, dtype=torch.int64, device=dev)
            g.send_ids = g.need_ids
            g.send_splits = [0] * g.world
            g.recv_splits = [0] * g.world
            g.local_adj = _unflatten(ls, ld, counts)
            g._flat = g._slot = g._mark = None
            if build_plan:
                g.build_plan()
            return g
        both = both[1:]
        g.recv_splits = [int(v) for v in both[: g.world]]            # halo rows I receive per owner
        g.send_splits = [int(v) for v in both[g.world: 2 * g.world]]  # rows I send per peer
        g.n_halo = sum(g.recv_splits)
        g.need_ids = need_buf[: g.n_halo]
        g._flat = g._local_flat = (ls, ld, counts)                   # `_flat` only serves `_type_ids` (device + counts)
        g.local_adj = _unflatten(ls, ld, counts)
        g._slot = g._mark = None
        if overlap:
            g.split_blocks([int(v) for v in both[2 * g.world:]])
        g._flat = None
        wanted = torch.empty(sum(g.send_splits), dtype=torch.int64, device=dev)
        dist.all_to_all_single(wanted, g.need_ids, g.send_splits, g.recv_splits, group=group)
        g.send_ids = wanted - g.lo                                    # owners trust their peers' requests
        if build_plan and not overlap:
            g.build_plan()
        return g

    def _index_pass(self, adjacency_lists: Adj, want_own_counts: bool):
        """The collective-free, host-read-free part of `build`: local ids of every endpoint (remote sources as
        n_local + their slot in the sorted distinct halo id list), that list, halo rows per owner, the number of
        remote-source edges, the halo total and (two-block mode) own-source edges per type -- all DEVICE tensors."""
        dev = adjacency_lists[0][0].device
        if dev.type == "cuda":
            # the whole index pass in HIP (csrc/shard_index.hip: 5 launches over the edge lists and a BITMAP of the
            # global id space, no host sync)
            ls, ld, counts, need_buf, sstats = ops.shard_index(adjacency_lists, self.lo, self.hi, self.bounds,
                                                               self.bounds_host[-1])
            w = self.world
            return (ls, ld, counts, need_buf, sstats[:w], sstats[w: w + 1], sstats[w + 1: w + 2], sstats[w + 2:])
        # gloo / CPU tests of the host logic: the same results from torch ops
        src, dst, counts = _flatten(adjacency_lists)
        rem = (src < self.lo) | (src >= self.hi)
        flag = rem.sum().reshape(1).to(torch.int64)
        need_counts = self.index_locally(adjacency_lists, (src, dst, counts))
        need_buf = torch.nonzero(self._mark, as_tuple=False).flatten()
        ls = torch.where(rem, self._slot[src].to(torch.int64) + self.n_local, src - self.lo)
        own = self.own_source_counts() if want_own_counts else None
        return ls, dst - self.lo, counts, need_buf, need_counts, flag, need_counts.sum().reshape(1), own

    def _finish_steady(self, planner: "ExchangePlanner", ls, ld, counts, need_buf, need_counts, group) -> None:
        """The rest of a build whose exchange sizes come from the planner's learned capacities (host integers known
        BEFORE this minibatch was looked at): halo table = [own rows | capacity block of owner 0 | of owner 1 | ...]."""
        dev = ls.device
        world, n = self.world, self.n_local
        R, S = planner.recv_caps, planner.send_caps
        self.global_stats = planner.global_stats          # one minibatch old: a speed decision, the same on every rank
        self.recv_splits, self.send_splits = list(R), list(S)
        self._slot = self._mark = self._flat = None
        if not planner.ever_cut:
            # no minibatch so far had a cut edge (the caller partitions on graph boundaries): predict the same -- no
            # exchange, no collective per layer.  A cut edge that does appear is an overflow (capacity 0) AND trips the
            # plan build's range guard (its source lies outside the own rows).
            self.no_cut, self.n_halo = True, 0
            self.need_ids = torch.zeros(0, dtype=torch.int64, device=dev)
            self.send_ids = self.need_ids
            self.local_adj = _unflatten(ls, ld, counts)
            return
        owner, off, caps = planner.layout(world, dev, self.bounds)
        total = sum(R)
        incl = torch.cumsum(need_counts, 0)
        prefix = incl - need_counts
        if total:
            j = torch.arange(total, dtype=torch.int64, device=dev) - off[owner]
            if need_buf.numel():
                pos = (prefix[owner] + j).clamp_(0, need_buf.numel() - 1)
                need_pad = torch.where(j < need_counts[owner], need_buf[pos], self.bounds[owner])
            else:
                need_pad = self.bounds[owner].clone()
        else:
            need_pad = torch.zeros(0, dtype=torch.int64, device=dev)
        # remote sources: n_local + slot in the dense halo list  ->  n_local + start of the owner's block + rank inside it
        slot = (ls - n).clamp_(min=0)
        q = torch.searchsorted(incl, slot, right=True).clamp_(max=world - 1)
        inside = torch.minimum(slot - prefix[q], (caps[q] - 1).clamp_(min=0))
        ls = torch.where(ls >= n, n + off[q] + inside, ls)
        self.n_halo = total
        self.need_ids = need_pad
        self.local_adj = _unflatten(ls, ld, counts)
        self._local_flat = (ls, ld, counts)
        wanted = torch.empty(sum(S), dtype=torch.int64, device=dev)
        dist.all_to_all_single(wanted, need_pad, list(S), list(R), group=group)
        self.send_ids = (wanted - self.lo).clamp_(0, max(n - 1, 0))   # padding asks for the owner's first row

    def attach_graph_index(self, node_to_graph_idx_local: torch.Tensor, num_graphs: int) -> "ShardedGraph":
        """`node_to_graph_idx` of the OWN rows (global graph ids, graphneuralnetwork.py:440-443,469-477) and the
        number of graphs in the whole batch: what the global-exchange layers pool over."""
        if node_to_graph_idx_local.shape[0] != self.n_local:
            raise ValueError("node_to_graph_idx must list exactly this rank's rows")
        self.node_to_graph_idx, self.num_graphs = node_to_graph_idx_local, int(num_graphs)
        return self

    def set_bounds(self, all_ranges, device) -> None:
        los = [int(r[0]) for r in all_ranges]
        his = [int(r[1]) for r in all_ranges]
        if any(a != b for a, b in zip(los[1:], his[:-1])) or (los[self.rank], his[self.rank]) != (self.lo, self.hi):
            raise ValueError("node ranges must be contiguous, ordered by rank and contain this rank's range")
        self.bounds_host = los + [his[-1]]
        self.bounds = _to_device_ints(self.bounds_host, device)

    def index_locally(self, adjacency_lists: Adj, flat=None) -> torch.Tensor:
        """The collective-free part of `build`: which halo rows this rank needs (de-duplicated, sorted, hence
        grouped by owner because the ranges are ordered).  Mark-and-compact over the global id space: one bool
        per node of the batch and one int32 prefix sum -- streaming passes at HBM speed (10 M nodes: 10 + 40 MB),
        against a sort of every remote endpoint for the alternative.  Returns the per-owner halo row counts as
        a DEVICE tensor; nothing here synchronises with the host."""
        src, dst, counts = flat if flat is not None else _flatten(adjacency_lists)
        dev = src.device
        total = self.bounds_host[-1]            # global node count
        mark = torch.zeros(total + 1, dtype=torch.bool, device=dev)
        mark.index_fill_(0, src, True)
        mark[self.lo:self.hi] = False           # own rows are not halo rows
        mark[total] = False
        self._slot = torch.cumsum(mark, 0, dtype=torch.int32) - mark.to(torch.int32)   # halo slot of every marked id
        self._mark = mark
        self._flat = (src, dst, counts)
        upto = self._slot[self.bounds].to(torch.int64)                # marked ids below each range boundary
        return (upto[1:] - upto[:-1]).contiguous()

    def finish_local_index(self) -> None:
        """After the split sizes are known on the host: the sorted halo ids and the edge endpoints remapped into
        the local table [own rows | halo rows] (one pass over the concatenated edge list; the per-type lists are
        views of it)."""
        dev = self._mark.device
        self.need_ids = (torch.nonzero(self._mark, as_tuple=False).flatten() if self.n_halo
                         else torch.zeros(0, dtype=torch.int64, device=dev))
        src, dst, counts = self._flat
        rem = (src < self.lo) | (src >= self.hi)
        ls = torch.where(rem, self._slot[src].to(torch.int64) + self.n_local, src - self.lo)
        ld = dst - self.lo
        self._local_flat = (ls, ld, counts)
        self.local_adj = _unflatten(ls, ld, counts)
        self._slot = self._mark = None

    def _type_ids(self) -> torch.Tensor:
        """Edge type of every edge of the concatenated list (int64 [E])."""
        src, _, counts = self._flat
        t = len(counts)
        return torch.repeat_interleave(torch.arange(t, dtype=torch.int64, device=src.device),
                                       _to_device_ints(counts, src.device), output_size=sum(counts))

    # -- two-block mode -----------------------------------------------------------------------------
    def own_source_counts(self) -> torch.Tensor:
        """int64 [T] on the device: edges per type whose source is an own row (after `index_locally`)."""
        src, _, counts = self._flat
        own = ((src >= self.lo) & (src < self.hi)).to(torch.int64)
        if len(counts) == 1:
            return own.sum().reshape(1)
        return torch.zeros(len(counts), dtype=torch.int64, device=src.device).index_add_(0, self._type_ids(), own)

    def split_blocks(self, own_counts: Sequence[int]) -> None:
        """Per type: own-source edges first, then halo-source edges (stable), as two adjacency lists over the SAME
        local table [own rows | halo rows]; one plan per block and the 2-slot plan that combines the two partial
        aggregates.  ONE stable sort of the concatenated list by (type, source-is-halo); the slices come from the
        host counts that travelled back with the split sizes: no further synchronisation."""
        n = self.n_local
        ls, ld, counts = self._local_flat
        key = (ls >= n).to(torch.int64)
        if len(counts) > 1:
            key = key + 2 * self._type_ids()
        order = torch.sort(key, stable=True).indices
        ls, ld = ls[order], ld[order]
        self.adj_own, self.adj_halo = [], []
        at = 0
        for c_all, c in zip(counts, own_counts):
            self.adj_own.append((ls[at: at + c], ld[at: at + c]))
            self.adj_halo.append((ls[at + c: at + c_all], ld[at + c: at + c_all]))
            at += c_all
        self.overlap = True
        if ls.is_cuda:
            rows = n + self.n_halo
            self.plan_own = ops.build_plan(self.adj_own, n, num_src_rows=rows)
            self.plan_halo = ops.build_plan(self.adj_halo, n, num_src_rows=rows)
            self.plan_comb = self._combine_plan(self.plan_own.rowptr, self.plan_halo.rowptr)

    def _combine_plan(self, rowptr_own: torch.Tensor, rowptr_halo: torch.Tensor) -> "ops.GraphPlan":
        """Plan over the stacked partial table [agg_own ; agg_halo] (2 n rows): row v reduces slot v if the own
        block has an edge into v and slot n + v if the halo block has one.  Blocks WITHOUT an edge into v are left
        out, so their torch_scatter-style 0 can never win a max over negative values; a row with no edge in either
        block stays empty and yields 0.  Built with prefix sums and scatters only (no host read-back)."""
        n = self.n_local
        dev = rowptr_own.device
        has_o = (rowptr_own[1:] > rowptr_own[:-1])
        has_h = (rowptr_halo[1:] > rowptr_halo[:-1])
        cnt = has_o.to(torch.int32) + has_h.to(torch.int32)
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        torch.cumsum(cnt, 0, out=rowptr[1:])
        v = torch.arange(n, dtype=torch.int64, device=dev)
        start = rowptr[:-1].to(torch.int64)
        col = torch.zeros(2 * n + 1, dtype=torch.int32, device=dev)       # last element: dump slot
        col.scatter_(0, torch.where(has_o, start, torch.full_like(start, 2 * n)), v.to(torch.int32))
        col.scatter_(0, torch.where(has_h, start + has_o.to(torch.int64), torch.full_like(start, 2 * n)),
                     (v + n).to(torch.int32))
        plan = ops.GraphPlan(rowptr, col, col, 0, n, 2 * n, 1)
        plan.num_src_rows = 2 * n
        return plan

    def begin_exchange(self, table: torch.Tensor):
        """Start the halo all-to-all into table[n_local:] (table[:n_local] holds this rank's rows) and return the
        work handle; `wait()` on it orders the CURRENT stream behind the arrival -- kernels launched in between
        (the own-source block) run while the rows travel over xGMI."""
        if self.no_cut:
            return None
        return dist.all_to_all_single(table[self.n_local:], self._send_rows(table), self.recv_splits, self.send_splits,
                                      group=self.group, async_op=True)

    def _send_rows(self, table: torch.Tensor) -> torch.Tensor:
        """The rows of this rank's block of `table` its peers asked for, in peer order (HIP row gather on the GPU)."""
        own = table[: self.n_local]
        if self.n_local == 0:      # (planner padding can reserve rows on a rank that owns none in this minibatch)
            return torch.zeros(self.send_ids.shape[0], table.shape[1], dtype=table.dtype, device=table.device)
        return ops.gather_rows(own, self.send_ids) if own.is_cuda else own.index_select(0, self.send_ids)

    @staticmethod
    def build_local(adjacency_lists: Adj, all_ranges: Sequence[Tuple[int, int]], rank: int,
                    overlap: bool = False, use_hip_index: bool = True) -> "ShardedGraph":
        """Collective-free construction of ONE rank's view (no process group): everything `build` derives from
        this rank's own edges -- halo ids, remapped adjacency, plan.  The send side (`send_ids`) needs the peers
        and stays empty, so this serves single-process simulations of a sharded run (tests, dry runs) where
        the caller supplies the halo rows."""
        g = ShardedGraph()
        g.rank, g.world = rank, len(all_ranges)
        g.lo, g.hi = int(all_ranges[rank][0]), int(all_ranges[rank][1])
        g.n_local = g.hi - g.lo
        g.set_bounds(all_ranges, adjacency_lists[0][0].device)
        g.no_cut = False
        if adjacency_lists[0][0].is_cuda and use_hip_index:
            ls, ld, counts, need_buf, sstats = ops.shard_index(adjacency_lists, g.lo, g.hi, g.bounds, g.bounds_host[-1])
            host = sstats.tolist()
            g.recv_splits = [int(v) for v in host[: g.world]]
            g.n_halo = sum(g.recv_splits)
            g.need_ids = need_buf[: g.n_halo]
            g._flat = g._local_flat = (ls, ld, counts)
            g.local_adj = _unflatten(ls, ld, counts)
            own_counts = [int(v) for v in host[g.world + 2:]] if overlap else None
        else:
            g.recv_splits = [int(v) for v in g.index_locally(adjacency_lists).tolist()]
            g.n_halo = sum(g.recv_splits)
            g.finish_local_index()
            own_counts = [int(v) for v in g.own_source_counts().tolist()] if overlap else None
        g.global_stats = (sum(int(a[0].shape[0]) for a in adjacency_lists), g.n_local, g.n_halo)
        g.send_splits = [0] * g.world
        g.send_ids = g.need_ids[:0]
        if adjacency_lists[0][0].is_cuda:
            g.build_plan()
        if overlap:
            g.split_blocks(own_counts)
        g._flat = None
        return g

    def build_plan(self) -> None:
        self._plan = ops.build_plan(self.local_adj, self.n_local, num_src_rows=self.n_local + self.n_halo)

    @property
    def plan(self) -> Optional["ops.GraphPlan"]:
        """The single-block plan over the local table; in two-block mode it is only built when a layer asks for
        it (training, mean aggregation)."""
        if self._plan is None and self.overlap and self.local_adj and self.local_adj[0][0].is_cuda:
            self.build_plan()
        return self._plan

    @property
    def num_edges(self) -> int:
        return sum(int(a[0].shape[0]) for a in self.local_adj)

    def form_sizes(self, rows_travel_as_states: bool) -> Tuple[int, int]:
        """(edges, table rows) the edge-form / table-form choice of a layer is made from: group-wide sums when the
        shard exchanges halo rows (one decision for all ranks), this rank's own sizes when nothing travels."""
        if self.no_cut or self.global_stats[1] == 0:
            return self.num_edges, self.n_local + (self.n_halo if rows_travel_as_states else 0)
        e, own, halo = self.global_stats
        return e, own + (halo if rows_travel_as_states else 0)

    # -- per-layer exchange -----------------------------------------------------------------------
    def new_table(self, dim: int, like: torch.Tensor) -> torch.Tensor:
        return torch.empty(self.n_local + self.n_halo, dim, dtype=like.dtype, device=like.device)

    def exchange_into(self, table: torch.Tensor) -> torch.Tensor:
        """table[:n_local] holds this rank's rows; fills table[n_local:] with the halo rows."""
        if self.no_cut:      # agreed on by every rank at build time: nobody enters the collective
            return table
        dist.all_to_all_single(table[self.n_local:], self._send_rows(table), self.recv_splits, self.send_splits,
                               group=self.group)
        return table

    def exchange(self, rows_local: torch.Tensor) -> torch.Tensor:
        if self.no_cut:      # the local table IS the own rows
            return rows_local
        table = self.new_table(rows_local.shape[1], rows_local)
        table[: self.n_local].copy_(rows_local)
        return self.exchange_into(table)

    def exchange_autograd(self, rows_local: torch.Tensor) -> torch.Tensor:
        """Differentiable `exchange`: backward is the transposed exchange -- the halo rows'
        gradients travel back to their owners over the same all-to-all with the splits swapped and are
        segment-summed onto the owners' rows (a row sent to several peers collects all of them)."""
        if self.no_cut:      # nothing travels in either direction
            return rows_local
        return _HaloExchange.apply(rows_local, self)

    def _send_plan(self):
        """Plan that sums returned gradient rows by the local row they belong to (built once per shard)."""
        if getattr(self, "_sp", None) is None:
            self._sp = ops.build_plan([(self.send_ids, self.send_ids)], self.n_local)
        return self._sp

    @property
    def halo_bytes_per_row_exchange(self) -> int:
        return 4 * sum(self.recv_splits)


class _HaloExchange(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows_local, shard):
        ctx.shard = shard
        return shard.exchange(rows_local)

    @staticmethod
    def backward(ctx, g):
        sh = ctx.shard
        g = g.contiguous()
        d_own = g[: sh.n_local]
        if sh.no_cut:   # agreed on by every rank at build time: nobody enters the collective
            return d_own, None
        back = torch.empty(sum(sh.send_splits), g.shape[1], dtype=g.dtype, device=g.device)
        dist.all_to_all_single(back, g[sh.n_local:].contiguous(), sh.send_splits, sh.recv_splits,
                               group=sh.group)
        if back.shape[0] == 0:
            return d_own, None
        if g.is_cuda:   # deterministic segment-sum on the HIP kernel
            extra = ops.segment_reduce(back, sh._send_plan(), "sum")
        else:           # gloo/CPU tests of the host logic only
            extra = torch.zeros_like(d_own).index_add_(0, sh.send_ids, back)
        return d_own + extra, None


OVERLAP_REDUCES = ("sum", "add", "max", "min")   # mean of partial means is not the mean: it takes the plain path


def aggregate_two_blocks(shard: "ShardedGraph", work, table_of, msg_dim: int, reduce: str, ydst=None, **epilogue):
    """The two-block aggregation of one layer (inference):

        work = shard.begin_exchange(...)                     halo rows start travelling
        part[:n] = aggregate(own-source block)               runs under the exchange
        work.wait()                                          current stream waits for the halo rows
        part[n:] = aggregate(halo-source block)
        out      = REDUCE over the (<= 2) non-empty partials of every row, with the row epilogue

    `table_of(block)` returns (message table, col, type_bits) for block "own" / "halo" -- called for "halo" only
    after the wait, so it may read the halo rows.  The combine is the same HIP gather/segment-reduce kernel over
    the stacked partial table: max / min stay exact; a sum becomes (own partial) + (halo partial), i.e. not the
    unsharded fold order (|delta| ~ 1e-7) -- which is why the mode is opt-in."""
    n = shard.n_local
    part = None
    for block, plan in (("own", shard.plan_own), ("halo", shard.plan_halo)):
        if block == "halo" and work is not None:
            work.wait()
        tab, col, tb = table_of(block)
        if part is None:
            part = torch.empty(2 * n, msg_dim, dtype=torch.float32, device=tab.device)
        ops.gather_reduce(tab, plan, msg_dim, reduce, ydst=ydst, col=col, type_bits=tb,
                          out=part[:n] if block == "own" else part[n:])
    return ops.gather_reduce(part, shard.plan_comb, msg_dim, reduce, type_bits=0, **epilogue)


# ------------------------------------------------------------------------------------------------
# bench / test helpers
# ------------------------------------------------------------------------------------------------
def make_weak_scaling_shard(nodes_per_rank: int, edges_per_rank: int, hidden: int, rank: int,
                            world: int, device, seed: int = 1234, cut_edges: bool = False) -> Dict:
    """Weak-scaling version of BASELINE config 2.  Rank p owns nodes [p N, (p+1) N) and their E
    in-edges of one batched graph of world * N nodes.
      cut_edges=False: a disjoint union of `world` random graphs partitioned on graph boundaries (the
                       shape of ptgnn's minibatches) -- no edge crosses a rank;
      cut_edges=True : ONE random graph, sources uniform over all world * N nodes, so (world-1)/world
                       of the edges are cut and every layer exchanges halo rows."""
    g = torch.Generator().manual_seed(seed + 7919 * rank)
    lo = rank * nodes_per_rank
    if cut_edges:
        src = torch.randint(0, world * nodes_per_rank, (edges_per_rank,), generator=g, dtype=torch.int64)
    else:
        src = torch.randint(0, nodes_per_rank, (edges_per_rank,), generator=g, dtype=torch.int64) + lo
    dst = torch.randint(0, nodes_per_rank, (edges_per_rank,), generator=g, dtype=torch.int64) + lo
    x = torch.randn(nodes_per_rank, hidden, generator=g, dtype=torch.float32)
    adj = [(src.to(device), dst.to(device))]
    return {"adj_global": adj, "range": (lo, lo + nodes_per_rank), "x": x.to(device),
            "all_ranges": [(p * nodes_per_rank, (p + 1) * nodes_per_rank) for p in range(world)]}


def layer_forward(layer, state: Dict) -> torch.Tensor:
    """One sharded message-passing layer: (re)build the shard plan for the minibatch, exchange halo
    rows, aggregate, update.  Nothing is cached across calls (bench.py times the whole thing)."""
    shard = ShardedGraph.build(state["adj_global"], state["range"], build_plan=False,
                               all_ranges=state.get("all_ranges"), overlap=state.get("overlap"),
                               planner=state.get("planner"))
    if shard.no_cut:   # no edge crosses a rank boundary: exactly the single-GPU layer on the local block
        return layer(state["x"], shard.local_adj, None, {}, {}, [None] * len(shard.local_adj))
    if not shard.overlap:
        shard.build_plan()
    return layer.forward_sharded(state["x"], shard)


def run_stack(layers: Sequence, x_local: torch.Tensor, shard: ShardedGraph) -> torch.Tensor:
    """The layer loop of GraphNeuralNetwork.gnn (graphneuralnetwork.py:122-131) over a sharded minibatch:
    message-passing and global-exchange layers take their `forward_sharded`; residual glue is node-local."""
    for layer in layers:
        if hasattr(layer, "forward_sharded"):
            x_local = layer.forward_sharded(x_local, shard)
        else:  # residual glue etc.: purely node-local
            x_local = layer(x_local, shard.local_adj, shard.node_to_graph_idx, {}, {},
                            [None] * len(shard.local_adj))
    return x_local


# ------------------------------------------------------------------------------------------------
# cross-rank combination of per-graph partial pools (global-exchange layers)
# ------------------------------------------------------------------------------------------------
class _AllReduce(torch.autograd.Function):
    """y = reduce over ranks of x (every rank gets y).  With the total loss = sum of the ranks' local losses:
    SUM : d x_r = sum over ranks of d y;   MAX/MIN: the same sum, routed to the rank(s) that hold the extremum."""

    @staticmethod
    def forward(ctx, x, op, group):
        y = x.contiguous().clone()
        dist.all_reduce(y, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX, "min": dist.ReduceOp.MIN}[op],
                        group=group)
        ctx.op, ctx.group = op, group
        if op != "sum":
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        dist.all_reduce(g, op=dist.ReduceOp.SUM, group=ctx.group)
        if ctx.op != "sum":
            x, y = ctx.saved_tensors
            g = g * (x == y).to(g.dtype)
        return g, None, None


def all_reduce(x: torch.Tensor, op: str, group=None) -> torch.Tensor:
    if dist.get_world_size(group) == 1:
        return x
    if torch.is_grad_enabled() and x.requires_grad:
        return _AllReduce.apply(x, op, group)
    y = x.contiguous().clone()
    dist.all_reduce(y, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX, "min": dist.ReduceOp.MIN}[op],
                    group=group)
    return y


def combine_graph_pools(partial: torch.Tensor, counts: torch.Tensor, kind: str, group=None) -> torch.Tensor:
    """Per-graph pools over the WHOLE batch from each rank's pool over its own nodes.
    partial [G, D]: this rank's sum (kind sum / mean) or max / min with torch_scatter's 0 for graphs it holds no
    node of; counts [G]: its node count per graph.  A graph that lives on one rank adds exact zeros (sum) or
    loses to -inf (max) elsewhere, so partitions on graph boundaries reproduce the unsharded pool bit for bit."""
    if kind in ("sum", "mean"):
        total = all_reduce(partial, "sum", group)
        if kind == "sum":
            return total
        n = all_reduce(counts.to(partial.dtype), "sum", group)
        return total / n.clamp(min=1).unsqueeze(1)
    if kind not in ("max", "min"):
        raise ValueError(kind)
    sentinel = float("-inf") if kind == "max" else float("inf")
    mine = counts > 0
    x = torch.where(mine.unsqueeze(1), partial, torch.full_like(partial, sentinel))
    y = all_reduce(x, kind, group)
    n = all_reduce(counts.to(torch.float32), "sum", group)
    return torch.where((n > 0).unsqueeze(1), y, torch.zeros_like(y))   # empty graphs pool to 0 (torch_scatter)
