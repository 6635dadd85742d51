"""Test support for the aggregation dispatch paths: a graph builder that places destination rows exactly at the
thresholds where the CSR aggregation kernels switch paths, and the float64 / serial-fp32 restatements the kernels are
compared with.  Never imported by the product package.

Thresholds (copied here; tests assert the ones the Python side exposes):
  * K_LONG_ROW = 256      ptgnn_amd/csrc/gather_reduce_core.h kLongRow: rows beyond it fold in k_long_rows (side path)
  * HUB_THRESHOLD = 2048  ptgnn_amd/ops.py HUB_THRESHOLD: rows beyond it take the chunked hub path
  * K_HUB_CHUNK = 1024    ptgnn_amd/csrc/gather_reduce_core.h kHubChunk: CSR slots per hub chunk
  * K_PNA_LONG = 256      ptgnn_amd/csrc/pna_aggregate.hip kPnaLong: rows beyond it get a workgroup (k_pna_long_rows)
  * UNROLL = 8 / 4        slots per prefetched group (4 with a destination term): degrees around multiples of 8 run
                          the clamped tail groups
"""
import torch

K_LONG_ROW = 256
HUB_THRESHOLD = 2048
K_HUB_CHUNK = 1024
K_PNA_LONG = 256
UNROLL = 8

# every in-degree the spectrum graph holds at least once
SPECTRUM_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 255, 256, 257, 258, 1023, 1024, 1025, 2047, 2048, 2049,
                    3073, 4097)


class Spectrum:
    """The layout of a degree-spectrum graph: N rows, the wanted in-degree of every row, the hub rows and the edge
    lists.  Built by `spectrum_graph`."""

    def __init__(self, deg, adj, hub_rows, shared_pair, hub_source, num_types):
        self.deg = deg                    # int64 [N] in-degree of every destination row
        self.adj = adj                    # [(src, dst)] per edge type (CPU int64), message order = type-major concat
        self.hub_rows = hub_rows          # rows with more than HUB_THRESHOLD in-edges
        self.shared_pair = shared_pair    # (r, r + 1): two hubs on adjacent rows
        self.hub_source = hub_source      # a source with more than HUB_THRESHOLD out-edges of type 0
        self.num_types = num_types

    @property
    def num_nodes(self):
        return int(self.deg.shape[0])

    @property
    def num_edges(self):
        return int(self.deg.sum())

    def rowptr(self):
        return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(self.deg, 0)])

    def src_dst_type(self):
        """Concatenated (src, dst, type) in message order."""
        src = torch.cat([s for s, _ in self.adj])
        dst = torch.cat([d for _, d in self.adj])
        typ = torch.cat([torch.full((s.shape[0],), t, dtype=torch.int64) for t, (s, _) in enumerate(self.adj)])
        return src, dst, typ

    def hub_chunks(self, row):
        """The hub chunks (CSR slots // K_HUB_CHUNK) row `row` touches."""
        rp = self.rowptr()
        return range(int(rp[row]) // K_HUB_CHUNK, (int(rp[row + 1]) - 1) // K_HUB_CHUNK + 1)


def spectrum_degrees(num_nodes=8192, background_max=6, seed=0):
    """In-degrees: the SPECTRUM_DEGREES spread over the rows (small ones several times), hubs at row 0, at row N-1 and
    on two adjacent rows in the middle, and a background of 0..background_max in-edges elsewhere.  The middle pair is
    moved by one row until its boundary slot is not a multiple of K_HUB_CHUNK, so the two hubs share a chunk."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, background_max + 1, (num_nodes,), generator=g)
    deg[0] = 3073
    deg[num_nodes - 1] = 2049
    special = []
    for d in SPECTRUM_DEGREES:
        special += [d] * (4 if d <= 17 else (2 if d <= 1025 else 1))
    rows = torch.randperm(num_nodes - 2000, generator=g)[: len(special)] + 1000   # away from both ends and the pair
    rows = rows[(rows < num_nodes // 2 - 8) | (rows > num_nodes // 2 + 8)]
    assert rows.shape[0] >= len(special) - 16
    for r, d in zip(rows.tolist(), special):
        deg[r] = d
    for d in SPECTRUM_DEGREES:                       # the filter above may have dropped one: put it back
        if not bool((deg == d).any()):
            deg[num_nodes // 2 + 20 + d % 7] = d
    pair = num_nodes // 2
    deg[pair], deg[pair + 1] = 4097, 2049
    if int(deg[: pair + 1].sum()) % K_HUB_CHUNK == 0:
        deg[pair - 1] += 1                       # a background row: the pair's boundary slot moves off the chunk edge
    return deg, (pair, pair + 1)


def spectrum_graph(num_types=1, num_nodes=8192, seed=0, hub_source_edges=2100):
    """Adjacency lists whose destination rows have exactly the `spectrum_degrees` in-degrees.  Edge order is shuffled
    (CSR slot order differs from message order), types are drawn at random, and node `hub_source` sends
    `hub_source_edges` (> HUB_THRESHOLD) edges of type 0, so the backward plan (rows = src * T + type) has a hub row."""
    deg, pair = spectrum_degrees(num_nodes, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    E = int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(num_nodes), deg)
    dst = dst[torch.randperm(E, generator=g)]
    src = torch.randint(0, num_nodes, (E,), generator=g)
    typ = torch.randint(0, num_types, (E,), generator=g)
    hub_source = 5
    t0 = torch.nonzero(typ == 0).flatten()
    pick = t0[torch.randperm(t0.shape[0], generator=g)[:hub_source_edges]]
    src[pick] = hub_source
    adj = [(src[typ == t].clone(), dst[typ == t].clone()) for t in range(num_types)]
    hubs = torch.nonzero(deg > HUB_THRESHOLD).flatten().tolist()
    return Spectrum(deg, adj, hubs, pair, hub_source, num_types)


def tie_values(rows, cols, seed):
    """fp32 [rows, cols] drawn from small integer sets that include -0.0 and +0.0: max / min tie inside rows, chunks
    and across chunk boundaries.  Column c % 3 == 1 is never positive (its max is a signed zero), c % 3 == 2 never
    negative (its min is a signed zero)."""
    g = torch.Generator().manual_seed(seed)
    sets = [torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]), torch.tensor([-2.0, -1.0, -0.0, 0.0]),
            torch.tensor([-0.0, 0.0, 1.0, 2.0])]
    out = torch.empty(rows, cols)
    for k in range(3):
        if k >= cols:
            break
        idx = torch.arange(k, cols, 3)
        if idx.numel():
            pick = torch.randint(0, sets[k].numel(), (rows, idx.numel()), generator=g)
            out[:, idx] = sets[k][pick]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def first_winner(msgs, dst, n, reduce):
    """torch_scatter's serial max / min (strict compare, the earliest message wins a tie): value bits and the winning
    message position (E for an empty row).  The value is the winner's own bits, so a tie of -0.0 and +0.0 returns the
    zero that comes first in message order."""
    from oracle import scatter_ref
    fn = scatter_ref.scatter_max if reduce == "max" else scatter_ref.scatter_min
    _, arg = fn(msgs, dst, 0, dim_size=n)
    E = msgs.shape[0]
    val = torch.where(arg < E, msgs.gather(0, arg.clamp(max=max(E - 1, 0))), torch.zeros((), dtype=msgs.dtype))
    return val, arg


def _winner(m, t, n, best):
    E, M = m.shape
    pos = torch.arange(E, device=m.device).unsqueeze(1).expand(E, M)
    cand = torch.where(m.detach() == best.index_select(0, t), pos, torch.full_like(pos, E))
    arg = torch.full((n, M), E, dtype=torch.int64, device=m.device)
    return arg.scatter_reduce_(0, t.unsqueeze(1).expand(E, M), cand, "amin", include_self=True)


def extreme(m, t, n, red):
    """Differentiable max / min (red = "amax" / "amin") with torch_scatter semantics: one winner, the first in message
    order; 0 for an empty row.  Any dtype, any device."""
    E, M = m.shape
    with torch.no_grad():
        best = torch.zeros(n, M, dtype=m.dtype, device=m.device).scatter_reduce_(
            0, t.unsqueeze(1).expand(E, M), m.detach(), red, include_self=False)
        arg = _winner(m, t, n, best)
    if E == 0:
        return torch.zeros(n, M, dtype=m.dtype, device=m.device)
    return torch.where(arg < E, m.gather(0, arg.clamp(max=E - 1)), torch.zeros((), dtype=m.dtype, device=m.device))


def segment_ref(m, t, n, reduce):
    """Differentiable torch_scatter reduce of [E, M] messages onto n rows in the dtype of `m`."""
    M = m.shape[1]
    if reduce in ("max", "min"):
        return extreme(m, t, n, "amax" if reduce == "max" else "amin")
    s = torch.zeros(n, M, dtype=m.dtype, device=m.device).index_add(0, t, m)
    if reduce == "mean":
        cnt = torch.zeros(n, dtype=m.dtype, device=m.device).index_add_(0, t, torch.ones_like(t, dtype=m.dtype))
        s = s / cnt.clamp(min=1).unsqueeze(1)
    return s


def pna_ref(m, t, n, delta):
    """pna_aggregation.py:27-56, the reference's operator sequence in the dtype of `m`."""
    M = m.shape[1]
    deg = torch.zeros(n, dtype=m.dtype, device=m.device).index_add_(0, t, torch.ones(t.shape[0], dtype=m.dtype,
                                                                                       device=m.device))
    s = torch.zeros(n, M, dtype=m.dtype, device=m.device).index_add(0, t, m)
    mean = s / (deg.unsqueeze(-1) + 1e-5)
    comp = torch.relu(m.pow(2) - mean[t].pow(2)) + 1e-10
    std = torch.sqrt(torch.zeros(n, M, dtype=m.dtype, device=m.device).index_add(0, t, comp))
    A = torch.cat([s, mean, extreme(m, t, n, "amax"), extreme(m, t, n, "amin"), std], dim=-1)
    s1 = torch.log(deg + 1).unsqueeze(-1) / delta
    return torch.cat([A, A * s1, A * (1 / (s1 + 1e-3))], dim=-1)


TOL = 1e-5


def attributed_ok(got, want32, exact, tol=TOL, scale=1.0):
    """The attributed bar (benchmarks/common.py attributed_parity): |got - fp32 reference| <= tol, or
    |got - float64| <= max(tol, 2 |fp32 reference - float64|) (all scaled)."""
    got, want32, exact = (torch.as_tensor(v).detach().double().cpu() for v in (got, want32, exact))
    if float((got - want32).abs().max()) <= tol * scale:
        return True
    ref_err = float((want32 - exact).abs().max())
    err = float((got - exact).abs().max())
    return err <= max(tol * scale, 2.0 * ref_err)
