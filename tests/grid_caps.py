"""Test support for the capped launch grids: one table entry per kernel whose host code caps the grid and covers the
rest of the work with a grid-stride loop, builders of the smallest input whose loop takes a SECOND trip (with witness
work at the first element of that trip, at its last element and in a ragged tail), and the plain restatements the GPU
tests compare with.  Never imported by the product package.

A grid of `cap` workgroups that each take `per_wg` work items per trip covers `threshold = cap * per_wg` items in the
first trip; item i >= threshold is reached only by a second trip.  tests/test_grid_caps_cpu.py reads every cap out of
the source text named here, so a changed cap fails there instead of silently un-covering tests/test_gpu_grid_caps.py.
"""
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ptgnn_amd", "csrc")

# kernels: the kernels behind the cap; file: under ptgnn_amd/csrc; pattern: a regex over the file's text whose groups
# are all the cap (searched with re.S; `hits` = how often it must occur); cap: workgroups (None: the number of compute
# units of the device, not a constant); per_wg: work items one workgroup takes per trip, in `unit`s; covered_by: the
# test that makes the second trip.
Cap = namedtuple("Cap", "kernels file pattern hits cap per_wg unit covered_by")

_NEW = "tests/test_gpu_grid_caps.py"

CAPS = {
    "validate": Cap(("k_validate",), "csr_build.hip",
                    r"k_validate<<<\(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\), 256,", 1, 2048, 256, "ids", _NEW),
    "shard": Cap(("k_shard_mark", "k_shard_remap"), "shard_index.hip",
                 r"const int64_t blocks = \(n \+ 255\) / 256;\s*launch\(tab, base, \(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\)\);",
                 1, 8192, 256, "edges of one table", _NEW),
    "uniq": Cap(("k_uniq_mark", "k_uniq_remap"), "shard_index.hip",
                r"const int64_t eblocks = \(num_edges \+ 255\) / 256;\s*const unsigned egrid = "
                r"\(unsigned\)\(eblocks < (\d+) \? \(eblocks > 0 \? eblocks : 1\) : (\d+)\);",
                1, 8192, 256, "CSR slots", _NEW),
    "gather_rows": Cap(("k_gather_rows",), "gather_reduce.hip",
                       r"int64_t blocks = \(n_idx \+ 3\) / 4;\s*if \(blocks > (\d+)\) blocks = (\d+);\s*k_gather_rows<<<",
                       1, 8192, 4, "rows", _NEW),
    "spread": Cap(("k_segment_spread",), "gather_reduce.hip",
                  r"int64_t blocks = \(items \+ 255\) / 256;\s*if \(blocks > (\d+)\) blocks = (\d+);\s*if \(vec4\)\s*"
                  r"k_segment_spread<true><<<", 1, 65536, 256, "items (slots x dim/4, or slots x dim scalar)", _NEW),
    "row_epilogue_backward": Cap(("k_row_epilogue_backward",), "row_epilogue.hip",
                                 r"constexpr int kMaxBackwardBlocks = (\d+);", 1, 2048, None,
                                 "rows (256 / LPR per workgroup)", _NEW),
    "pna_long": Cap(("k_pna_long_rows", "k_pna_bwd_long_rows"), "pna_aggregate.hip",
                    r"const int64_t lb = \(a\.num_nodes \+ 255\) / 256;\s*dim3 lgrid\(\(unsigned\)\(lb < (\d+) \? lb : (\d+)\),",
                    1, 1024, 256, "rows scanned", _NEW),
    "long_rows": Cap(("k_long_rows",), "gather_reduce_core.h",
                     r"const int64_t lb = \(a\.num_nodes - a\.row_begin \+ 255\) / 256;\s*"
                     r"dim3 lgrid\(\(unsigned\)\(lb < (\d+) \? lb : (\d+)\),", 1, 2048, 256, "rows scanned", _NEW),
    "hub_chunks": Cap(("k_hub_chunks",), "gather_reduce_core.h",
                      r"dim3 hgrid\(\(unsigned\)\(chunks < (\d+) \? chunks : (\d+)\),", 2, 1024, 1,
                      "(chunk, row) entries of the hub list", _NEW),
    "char": Cap(("k_char_embed", "k_window_max", "k_window_max_backward"), "char_conv.hip",
                r"inline unsigned grid_for\(int64_t items\) \{\s*int64_t blocks = \(items \+ 255\) / 256;\s*"
                r"if \(blocks > (\d+)\) blocks = (\d+);", 1, 65536, 256, "items", _NEW),
    # ---- the plan build's small capped kernels -------------------------------------------------------------------------
    "max_degree": Cap(("k_max_degree",), "csr_build.hip",
                      r"k_max_degree<<<\(unsigned\)\(mb < (\d+) \? mb : (\d+)\), 256,", 1, 1024, 256, "rows", _NEW),
    "pack": Cap(("k_pack",), "csr_build.hip", r"k_pack<<<\(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\), 256,", 1, 4096,
                256, "edges of one table of 64 edge types", _NEW),
    "zero_rowptr": Cap(("k_zero_rowptr",), "csr_build.hip",
                       r"k_zero_rowptr<<<\(unsigned\)\(zb < (\d+) \? zb : (\d+)\), 256,", 1, 1024, 256, "rowptr entries",
                       _NEW),
    "hub_list": Cap(("k_hub_list",), "csr_build.hip",
                    r"k_hub_list<<<\(unsigned\)\(hb < (\d+) \? hb : (\d+)\), 256,", 2, 2048, 256, "rows", _NEW),
    # ---- covered by the tests of their own families ---------------------------------------------------------------------
    "gru_gates_backward": Cap(("k_gru_gates_backward",), "dense_f32.hip",
                              r"if \(blocks > (\d+)\) blocks = (\d+);\s*k_gru_gates_backward<<<", 1, 65536, 256,
                              "float4 items", "tests/test_gpu_dense_paths.py::test_gru_gates_backward_grid_stride_wrap"),
    "half_gru_ws": Cap(("k_half_gru_ws",), "half_gemm.hip",
                       r"const unsigned grid = \(unsigned\)\(num_panels < cus \? num_panels : cus\);", 1, None, 1,
                       "row panels", "tests/test_gpu_half_inputs.py::test_more_row_panels_than_workgroups"),
    "edge16": Cap(("k_edge16_ws", "k_edge16"), "edge_gemm16.hip",
                  r"if \(units >= 0 && units < grid\) grid = units;\s*k_edge16_ws<", 1, None, 1, "32-row units",
                  "tests/test_gpu_edge_inputs.py::test_more_units_than_workgroups"),
}

# lane groups per workgroup of k_row_epilogue_backward = 256 / LPR (row_epilogue.hip `dispatch`)
ROW_EPILOGUE_BLOCK = 256


def row_epilogue_rows_per_wg(dim, vec4=None):
    """Rows one workgroup of k_row_epilogue_backward takes per trip at width `dim` (contiguous, aligned rows)."""
    vec4 = dim % 4 == 0 if vec4 is None else vec4
    if vec4:
        lpr = 16 if dim <= 64 else 32 if dim <= 128 else 64
    else:
        lpr = 64
    return ROW_EPILOGUE_BLOCK // lpr


def row_epilogue_route(dim):
    """(VEC, LPR, CH) of row_epilogue.hip `dispatch` for contiguous, aligned rows."""
    if dim % 4 == 0:
        return (4, 16, 1) if dim <= 64 else (4, 32, 1) if dim <= 128 else (4, 64, 1) if dim <= 256 else (4, 64, 2)
    return (1, 64, 1) if dim <= 64 else (1, 64, 4) if dim <= 256 else (1, 64, 8)


def threshold(name, per_wg=None):
    c = CAPS[name]
    return c.cap * (c.per_wg if per_wg is None else per_wg)


def source_caps(name):
    """The cap constants as they stand in the source text: one tuple of ints per match of the entry's pattern."""
    c = CAPS[name]
    text = open(os.path.join(CSRC, c.file)).read()
    return [tuple(int(g) for g in m.groups()) for m in re.finditer(c.pattern, text, flags=re.S)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. index guard
# ---------------------------------------------------------------------------------------------------------------------
def validate_case(n_ids=700_000, num_nodes=1000, seed=1):
    """ids [n_ids] int64 inside [0, num_nodes) except three planted ones, all in the second trip: a negative id at its
    first element, an id == num_nodes in the middle and an id past num_nodes as the very last (ragged tail) id."""
    g = torch.Generator().manual_seed(seed)
    clean = torch.randint(0, num_nodes, (n_ids,), generator=g)
    thr = threshold("validate")
    bad = clean.clone()
    planted = {thr: -3, (thr + n_ids) // 2: num_nodes, n_ids - 1: num_nodes + 7}
    for pos, v in planted.items():
        bad[pos] = v
    return dict(clean=clean, bad=bad, planted=planted, num_nodes=num_nodes, size=n_ids, per_wg=256,
                witness=sorted(planted))


def count_bad(ids, num_nodes):
    return int(((ids < 0) | (ids >= num_nodes)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 2. shard index
# ---------------------------------------------------------------------------------------------------------------------
def shard_case(num_edges=2_200_000, seed=2):
    """One edge table of `num_edges` edges that all end in rank 1's destination range; sources spread over the three
    ranks.  Two remote sources occur ONLY in the second trip: `first_id` at its first edge and `last_id` at the last
    edge of the table (a ragged tail: num_edges is no multiple of 256)."""
    g = torch.Generator().manual_seed(seed)
    ranges = [(0, 10_000), (10_000, 20_000), (20_000, 30_000)]
    total = ranges[-1][1]
    first_id, last_id = total - 1, 3                      # owned by rank 2 and by rank 0
    src = torch.randint(0, total, (num_edges,), generator=g)
    src[src == first_id] = first_id - 1
    src[src == last_id] = last_id + 1
    dst = torch.randint(ranges[1][0], ranges[1][1], (num_edges,), generator=g)
    thr = threshold("shard")
    src[thr], src[num_edges - 1] = first_id, last_id
    return dict(adj=[(src, dst)], ranges=ranges, rank=1, total=total, size=num_edges, per_wg=256,
                witness=[thr, num_edges - 1], witness_ids=[first_id, last_id])


# ---------------------------------------------------------------------------------------------------------------------
# 3. unique (edge type, source) pairs
# ---------------------------------------------------------------------------------------------------------------------
def csr_order(adj, num_nodes):
    """(perm, rows) of the plan's CSR: perm[slot] = position of the slot's edge in the type-major concatenation (a
    stable sort by destination), rows[slot] = its destination row."""
    dst = np.concatenate([d.numpy() for _, d in adj])
    perm = np.argsort(dst, kind="stable")
    return perm, dst[perm]


def unique_case(counts=(1_500_000, 700_000), num_nodes=70_001, seed=3):
    """Two edge types over `num_nodes` nodes.  Sources are drawn below num_nodes - 2; the two ids above occur once each:
    num_nodes - 1 (type 0) on the edge that lands in the FIRST CSR slot of the second trip, num_nodes - 2 (type 1) on the
    edge of the LAST CSR slot -- so those two (type, source) pairs exist only in the second trip."""
    g = torch.Generator().manual_seed(seed)
    adj = [(torch.randint(0, num_nodes - 2, (c,), generator=g), torch.randint(0, num_nodes, (c,), generator=g))
           for c in counts]
    E, thr = sum(counts), threshold("uniq")
    perm, rows = csr_order(adj, num_nodes)
    # the first slot of a row holds the row's earliest type-0 edge: take the first row that STARTS in the second trip
    starts = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
    s_first = int(starts[np.searchsorted(starts, thr)])
    e_first, e_last = int(perm[s_first]), int(perm[E - 1])
    assert e_first < counts[0] <= e_last, "the witness edges must be of type 0 and of type 1"
    adj[0][0][e_first] = num_nodes - 1
    adj[1][0][e_last - counts[0]] = num_nodes - 2
    return dict(adj=adj, num_nodes=num_nodes, size=E, per_wg=256, witness=[s_first, E - 1],
                witness_pairs=[(0, num_nodes - 1), (1, num_nodes - 2)])


def unique_ref(adj, num_nodes, type_bits, col):
    """numpy restatement of ptgnn_amd_unique_sources: (sorted distinct sources per type, slot_row [E], counts [T + 1])
    for the plan's col array ((src << type_bits) | type)."""
    want = [np.unique(a[0].numpy()) for a in adj]
    off = np.cumsum([0] + [len(w) for w in want])
    col = np.asarray(col).astype(np.int64)
    typ, src = col & ((1 << type_bits) - 1), col >> type_bits
    rows = np.empty(col.shape[0], dtype=np.int64)
    for t, w in enumerate(want):
        sel = typ == t
        rows[sel] = off[t] + np.searchsorted(w, src[sel])
    return want, rows, np.array([len(w) for w in want] + [off[-1]], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 4. gather_rows
# ---------------------------------------------------------------------------------------------------------------------
def gather_rows_case(table_rows=1000, seed=4):
    """idx [32,768 + 3]: the second trip is three rows (its workgroup runs three of its four waves); they read the last
    row of the table, a random one and row 0."""
    n = threshold("gather_rows") + 3
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, table_rows, (n,), generator=g)
    idx[n - 3], idx[n - 1] = table_rows - 1, 0
    return dict(idx=idx, table_rows=table_rows, size=n, per_wg=4, witness=[n - 3, n - 2, n - 1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. generic spread
# ---------------------------------------------------------------------------------------------------------------------
SPREAD_SHAPES = {3: 5_592_406, 260: 258_112}     # dim -> CSR slots; items = slots * dim (scalar) / slots * dim / 4 (float4)


def spread_items(dim, slots):
    return slots * (dim // 4 if dim % 4 == 0 else dim)


def spread_case(dim, num_nodes=1000, seed=5):
    """One edge type of SPREAD_SHAPES[dim] edges onto `num_nodes` rows; `arg` [num_nodes, dim] names for every (row,
    column) one CSR slot of the row (-1 for an empty row), as the max / min forward records its winners."""
    slots = SPREAD_SHAPES[dim]
    g = torch.Generator().manual_seed(seed + dim)
    dst = torch.randint(0, num_nodes, (slots,), generator=g)
    dst[0] = num_nodes - 1                      # the table's last row has an edge: the last CSR slot is a real row's
    src = torch.zeros(slots, dtype=torch.int64)
    perm, rows = csr_order([(src, dst)], num_nodes)
    deg = np.bincount(rows, minlength=num_nodes)
    rowptr = np.r_[0, np.cumsum(deg)]
    pick = torch.rand(num_nodes, dim, generator=g).numpy()
    arg = (rowptr[:-1, None] + np.floor(pick * deg[:, None])).astype(np.int64)
    arg = np.where(deg[:, None] > 0, np.minimum(arg, rowptr[1:, None] - 1), -1).astype(np.int32)
    arg[rows[slots - 1], :] = slots - 1         # the last slot wins every column of its row: its items carry gradient
    items = spread_items(dim, slots)
    return dict(adj=[(src, dst)], num_nodes=num_nodes, dim=dim, slots=slots, perm=perm, rows=rows,
                arg=torch.from_numpy(arg), size=items, per_wg=256, witness=[threshold("spread"), items - 1])


def spread_ref(grad, arg, perm, rows):
    """Index restatement of ptgnn_amd_segment_spread_f32: out[perm[s], c] = grad[rows[s], c], and with `arg` only where
    arg[rows[s], c] == s (zero elsewhere).  grad [N, D] fp32 numpy; returns [E, D] fp32."""
    out = np.empty((perm.shape[0], grad.shape[1]), dtype=np.float32)
    val = grad[rows]
    if arg is not None:
        val = np.where(arg[rows] == np.arange(perm.shape[0], dtype=np.int64)[:, None], val, np.float32(0))
    out[perm] = val
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 6. row epilogue
# ---------------------------------------------------------------------------------------------------------------------
# 130 and 301 take the two scalar routes no other test launches (widths off four above 64: CH = 4 up to 256, CH = 8 beyond)
ROW_EPILOGUE_SHAPES = [(32_768 + 17, 64), (16_384 + 9, 128), (8_192 + 5, 256), (8_192 + 5, 512), (8_192 + 5, 50),
                       (8_192 + 5, 300), (8_192 + 5, 130), (8_192 + 5, 301)]
ROW_EPILOGUE_FLAGS = {"gelu": 1, "ln": 2, "gelu_ln": 3}      # ops.EPI_GELU | ops.EPI_LAYERNORM


def row_epilogue_case(rows, dim, flags, seed=6):
    g = torch.Generator().manual_seed(seed + rows + 7 * dim + len(flags))
    x = torch.randn(rows, dim, generator=g) * 1.5
    gy = torch.randn(rows, dim, generator=g)
    gamma = torch.randn(dim, generator=g) if "ln" in flags else None
    beta = torch.randn(dim, generator=g) if "ln" in flags else None
    per = row_epilogue_rows_per_wg(dim)
    return dict(x=x, gy=gy, gamma=gamma, beta=beta, size=rows, per_wg=per,
                witness=[threshold("row_epilogue_backward", per), rows - 1])


def row_epilogue_ref(x, gy, gamma, beta, flags, dtype, eps=1e-5):
    """(y, grad_x, grad_gamma, grad_beta) of LayerNorm(GELU(x)) (`flags`: which of the two) by torch autograd on the CPU
    in `dtype`; the last two are None without LayerNorm."""
    xr = x.detach().to(dtype).requires_grad_(True)
    leaves = [xr]
    y = torch.nn.functional.gelu(xr) if "gelu" in flags else xr
    if "ln" in flags:
        ga, be = gamma.detach().to(dtype).requires_grad_(True), beta.detach().to(dtype).requires_grad_(True)
        leaves += [ga, be]
        y = torch.nn.functional.layer_norm(y, (x.shape[1],), ga, be, eps)
    y.backward(gy.to(dtype))
    grads = [t.grad for t in leaves] + [None] * (3 - len(leaves))
    return (y.detach(), *grads)


def row_epilogue_plain(x, gy, gamma, beta, flags, eps=1e-5):
    """The same four arrays written out in float64 numpy (erf GELU, biased variance), without autograd."""
    x, gy = x.double().numpy(), gy.double().numpy()
    erf = np.vectorize(math.erf)
    h = 0.5 * x * (1.0 + erf(x / math.sqrt(2.0))) if "gelu" in flags else x
    dh = gy
    y, gg, gb = h, None, None
    if "ln" in flags:
        ga, be = gamma.double().numpy(), beta.double().numpy()
        mean = h.mean(1, keepdims=True)
        rstd = 1.0 / np.sqrt(((h - mean) ** 2).mean(1, keepdims=True) + eps)
        xhat = (h - mean) * rstd
        y = xhat * ga + be
        gg, gb = (gy * xhat).sum(0), gy.sum(0)
        dxh = gy * ga
        dh = rstd * (dxh - dxh.mean(1, keepdims=True) - xhat * (dxh * xhat).mean(1, keepdims=True))
    if "gelu" in flags:
        dh = dh * (0.5 * (1.0 + erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))
    return y, dh, gg, gb


# ---------------------------------------------------------------------------------------------------------------------
# 7. PNA long rows
# ---------------------------------------------------------------------------------------------------------------------
def pna_case(M, seed=7, background=3000):
    """N = 262,144 + 300 rows; rows of 257 and 300 in-edges at row 5, at the last row of the first trip, at the first two
    rows of the second trip and at row N - 1; `background` short rows' edges elsewhere; every other row is empty.
    Returns the messages in a shuffled order, their targets, and the compact restatement of the non-empty rows (PNA
    is row-wise: `live` rows renumbered 0 .. len(live) - 1, same message order)."""
    thr = threshold("pna_long")
    N = thr + 300
    long_rows = {5: 300, thr - 1: 257, thr: 257, thr + 1: 300, N - 1: 300}
    g = torch.Generator().manual_seed(seed + M)
    t = torch.cat([torch.full((d,), r, dtype=torch.int64) for r, d in long_rows.items()]
                  + [torch.randint(0, N, (background,), generator=g)])
    t = t[torch.randperm(t.shape[0], generator=g)]
    m = torch.randn(t.shape[0], M, generator=g)
    live, compact = torch.unique(t, return_inverse=True)
    gout = torch.randn(live.shape[0], 15 * M, generator=g)
    return dict(messages=m, targets=t, num_nodes=N, live=live, compact=compact, gout=gout, long_rows=long_rows,
                size=N, per_wg=256, witness=[r for r in long_rows if r >= thr])


# ---------------------------------------------------------------------------------------------------------------------
# 8. hub list and long rows of the CSR aggregation
# ---------------------------------------------------------------------------------------------------------------------
K_HUB_CHUNK = 1024


def small_int_messages(E, M, seed):
    """fp32 [E, M] of integers in [-4, 4]: every partial sum of fewer than 2^22 of them is an integer below 2^24, so sum,
    max and min are exact in fp32 whatever the fold order.  Column 0 is all ones (a row's sum is its in-degree: a chunk
    that is skipped or folded twice always shows), columns 1 and 2 stay below 4 (the tests plant their one 4)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-4, 5, (E, M), generator=g).float()
    m[:, 0] = 1.0
    m[:, 1:3] = m[:, 1:3].clamp(max=3.0)
    return m


def hub_entries_of(deg):
    """(chunk, row) entries the plan's hub list holds for in-degrees `deg` (rows beyond 2048 in-edges), in row order --
    the device list has the same entries in any order."""
    rowptr = np.r_[0, np.cumsum(np.asarray(deg, dtype=np.int64))]
    out = []
    for r in np.flatnonzero(np.asarray(deg) > 2048):
        out += [(c, int(r)) for c in range(int(rowptr[r]) // K_HUB_CHUNK, int(rowptr[r + 1] - 1) // K_HUB_CHUNK + 1)]
    return out


def _graph_from_degrees(deg, seed):
    g = torch.Generator().manual_seed(seed)
    N, E = deg.shape[0], int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(N), deg)
    dst = dst[torch.randperm(E, generator=g)]
    src = torch.randint(0, N, (E,), generator=g)
    return src, dst


def hub_case(seed=8):
    """8(a): E < 2^21 (one stream).  Row 7 of 64 holds 1,100,000 in-edges -- 1,075 or 1,076 hub-list entries, more than
    the 1,024 workgroups of the dedicated hub launch; the other rows share 5,000 edges."""
    N = 64
    g = torch.Generator().manual_seed(seed)
    deg = torch.bincount(torch.randint(0, N, (5000,), generator=g), minlength=N)
    deg[7] = 1_100_000
    src, dst = _graph_from_degrees(deg, seed + 1)
    entries = hub_entries_of(deg.numpy())
    return dict(adj=[(src, dst)], deg=deg, num_nodes=N, hub_row=7, entries=entries, size=len(entries), per_wg=1,
                witness=[threshold("hub_chunks"), len(entries) - 1])


def side_stream_case(seed=9):
    """8(b): E >= 2^21 (hub chunks and long rows on the side streams), N = 524,288 + 600.  One hub of 1,200,000 in-edges
    at row N - 2 (past the 262,144 rows of k_max_degree's first trip: it is the plan's maximum degree); long rows of 257
    to 2,048 in-edges at row 100, at the last row of k_long_rows' first trip, at the first rows of its second trip and at
    row N - 1; 900,000 background edges."""
    thr = threshold("long_rows")
    N = thr + 600
    g = torch.Generator().manual_seed(seed)
    deg = torch.bincount(torch.randint(0, N, (900_000,), generator=g), minlength=N)
    long_rows = {100: 300, thr - 1: 257, thr: 257, thr + 1: 2048, thr + 63: 1024, thr + 64: 300, N - 1: 1025}
    for r, d in long_rows.items():
        deg[r] = d
    deg[N - 2] = 1_200_000
    src, dst = _graph_from_degrees(deg, seed + 1)
    entries = hub_entries_of(deg.numpy())
    return dict(adj=[(src, dst)], deg=deg, num_nodes=N, hub_row=N - 2, long_rows=long_rows, entries=entries,
                size=N, per_wg=256, witness=[r for r in long_rows if r >= thr],
                hub_size=len(entries), hub_witness=[threshold("hub_chunks"), len(entries) - 1],
                max_degree_row=N - 2)


def segment_ref64(msgs, dst, n, reduce):
    """float64 sum / mean of [E, M] messages onto n rows (index_add; empty rows 0)."""
    m = msgs.double()
    s = torch.zeros(n, m.shape[1], dtype=torch.float64).index_add_(0, dst, m)
    if reduce == "mean":
        s = s / torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 9. char-CNN kernels
# ---------------------------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def char_embed_case(seed=10):
    """k_char_embed: one thread per 4 columns of an output row, items = B R dim / 4 -- the output is 16 bytes per item
    whatever the shape, so the smallest input has the fewest rows.  dim = 1020 (255 items per row: a workgroup of 256
    straddles rows and the last one is ragged; 1024 is the kernel's limit), window 2 over L = 4 characters (R = 3)."""
    C, L, W, dim = 7, 4, 2, 1020
    R, q = L - W + 1, dim // 4
    thr = threshold("char")
    B = _ceil_div(_ceil_div(thr + 1, q), R) + 1
    g = torch.Generator().manual_seed(seed)
    chars = torch.randint(0, C, (B, L), generator=g)
    w1 = torch.randn(dim, C, W, generator=g) * 0.5          # nn.Conv1d weight [F, C, k]
    b1 = torch.randn(dim, generator=g) * 0.5
    items = B * R * q
    return dict(chars=chars, w1=w1, b1=b1, C=C, L=L, W=W, R=R, dim=dim, B=B, size=items, per_wg=256,
                witness=[thr, items - 1], first_row=thr // q)


def char_table(w1):
    """The [k C, F] table of ops.char_embed from the Conv1d weight [F, C, k]."""
    F, C, k = w1.shape
    return w1.permute(2, 1, 0).reshape(k * C, F).contiguous()


def window_max_case(seed=11):
    """k_window_max: items = B dim (scalar columns: dim = 255 is no multiple of 4), two rows per sample -- the smallest
    frame with a maximum to take.  Small integers: every column has tied rows somewhere (the lowest position wins)."""
    dim, R = 255, 2
    thr = threshold("char")
    B = _ceil_div(thr + 1, dim) + 5
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B * R, dim), generator=g).float()
    return dict(x=x, B=B, R=R, dim=dim, size=B * dim, per_wg=256, witness=[thr, B * dim - 1], first_row=thr // dim)


def window_max_ref(x, B, R, valid):
    """(max, lowest winning position) over the first `valid` rows of every sample's R-row frame, in float64."""
    f = x.double().reshape(B, R, -1)[:, :valid]
    best = f.max(dim=1)[0]
    first = (f == best.unsqueeze(1)).to(torch.uint8).argmax(dim=1)       # the first position that attains the maximum
    return best, first


def window_max_backward_case(seed=12):
    """k_window_max_backward: items = B R dim (scalar columns, dim = 255), R = 2."""
    dim, R = 255, 2
    thr = threshold("char")
    B = _ceil_div(_ceil_div(thr + 1, dim), R) + 3
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(B, dim, generator=g) + 3.0
    arg = torch.randint(0, R, (B, dim), generator=g).to(torch.int32)
    items = B * R * dim
    return dict(grad=grad, arg=arg, B=B, R=R, dim=dim, size=items, per_wg=256, witness=[thr, items - 1],
                first_row=thr // dim)


def window_max_backward_ref(grad, arg, R):
    """[B R, D]: grad[b, d] at row arg[b, d] of sample b, zeros elsewhere."""
    B, D = grad.shape
    out = torch.zeros(B, R, D, dtype=grad.dtype)
    out.scatter_(1, arg.long().unsqueeze(1), grad.unsqueeze(1))
    return out.reshape(B * R, D)


# ---------------------------------------------------------------------------------------------------------------------
# 10. the plan build's small capped kernels
# ---------------------------------------------------------------------------------------------------------------------
def pack_case(num_nodes=5000, seed=13):
    """k_pack narrows the lists of a plan with more than 64 edge types, 64 types per launch: 65 types whose first 64
    hold 1,048,576 + 362 edges (type 0 almost all of them, types 1..63 one edge each -- the last item of the launch is
    type 63's edge), and a 65th type of ten edges for the second launch."""
    thr = threshold("pack")
    counts = [thr + 299] + [1] * 63 + [10]
    g = torch.Generator().manual_seed(seed)
    adj = [(torch.randint(0, num_nodes, (c,), generator=g), torch.randint(0, num_nodes, (c,), generator=g))
           for c in counts]
    first_table = sum(counts[:64])
    return dict(adj=adj, num_nodes=num_nodes, size=first_table, per_wg=256, witness=[thr, first_table - 1])


def plan_ref(adj, type_bits):
    """(rowptr-free) numpy restatement of a forward plan: (perm, rows, col) in CSR slot order."""
    perm, rows = csr_order(adj, None)
    src = np.concatenate([s.numpy() for s, _ in adj])
    typ = np.concatenate([np.full(s.shape[0], t, dtype=np.int64) for t, (s, _) in enumerate(adj)])
    return perm, rows, (src[perm] << type_bits) | typ[perm]


def zero_rowptr_case():
    """An edge-free plan of 262,144 + 300 rows: k_zero_rowptr's second trip writes rowptr[262,144 ..]."""
    n = threshold("zero_rowptr") + 300
    return dict(num_nodes=n, size=n + 1, per_wg=256, witness=[threshold("zero_rowptr"), n])


def hub_list_case():
    """A sorted segment index over 524,288 + 600 segments (ops.plan_from_sorted_index -> ptgnn_amd_hub_list): segments
    of 3,000 elements at segment 7, at the first segment of k_hub_list's second trip and at the last segment; one
    element in every 64th other segment."""
    thr = threshold("hub_list")
    n = thr + 600
    deg = torch.zeros(n, dtype=torch.int64)
    deg[::64] = 1
    hubs = [7, thr, n - 1]
    for r in hubs:
        deg[r] = 3000
    index = torch.repeat_interleave(torch.arange(n), deg)
    return dict(index=index, deg=deg, num_segments=n, entries=hub_entries_of(deg.numpy()), size=n, per_wg=256,
                witness=[thr, n - 1])
