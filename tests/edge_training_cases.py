"""Test support for the opt-in 16-bit matrix inputs of the GGNN EDGE-FORM training step (`matrix_inputs(dt,
edge_training=True)`; csrc/edge_gemm16.hip's masked forms, csrc/edge_wgrad16.hip): float64 restatements of the masked
per-edge forward, its input gradient and the per-type weight gradient on ROUNDED operands, the mask unpacked from its
bits, and case builders.  Reference, bar and margin are those of tests/half_cases.py and tests/half_training_cases.py
(imported, not repeated).  Never imported by the product package.

The reference rounds what the kernels round.  Forward and weight gradient: `(x.float() * scale32)` with the scale
1 / (1 - p) computed in fp32, zero where the element is dropped, THEN the one rounding -- as autocast applies nn.Dropout
before the 16-bit Linear.  Input gradient: the product of the rounded operands, then mask and scale (on the fp32
accumulator in the kernel, in float64 here: one more fp32 rounding, 6e-8 relative, far inside the bar).
"""
import torch

import half_cases as C
import half_training_cases as T

P = 0.25
SEED = 4242                                # of the GPU tests' dropout mask (`hash_keep` restates it on the CPU)
N = 50                                     # nodes
COUNTS = (0, 1, 31, 33, 70)                # an empty type, a single row, units on either side of 32
EDGE_SHAPES = ((64, 64), (128, 128), (96, 160))     # (H, M): weight-stationary KS = 4, 8; per-wave, ragged column group
WGRAD_SHAPES = ((32, 32), (96, 160), (128, 128))    # (H, M)
MASKED_FAMILIES = ("edge16_masked", "edge_wgrad16")
FP32_EDGE_FAMILIES = ("k_stream_edge", "k_stream_edge_shared", "k_stream_edge_v2", "k_edge_linear")
FP32_WGRAD_FAMILIES = ("k_edge_wgrad", "k_wgrad_stream")


def scale32(p: float) -> float:
    """1.0f / (1.0f - p) as the kernels and make_dropout compute it: in fp32."""
    return float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32)
                                                           - torch.tensor(p, dtype=torch.float32)))


def unpack(bits: torch.Tensor, width: int) -> torch.Tensor:
    """The keep mask [rows, width] (bool, CPU) of int32 [rows, width / 32] words: bit b of word c = column 32 c + b."""
    words = bits.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    keep = (words.unsqueeze(-1) >> torch.arange(32, dtype=torch.int64)) & 1
    return keep.reshape(bits.shape[0], -1)[:, :width].bool()


def _mix32(x: torch.Tensor) -> torch.Tensor:
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x21F0AAAD) & m
    x = x ^ (x >> 15)
    x = (x * 0x735A2D97) & m
    return x ^ (x >> 15)


def hash_keep(rows: int, width: int, p: float, seed: int) -> torch.Tensor:
    """The keep mask of `ops.dropout_bitmask(rows, width, p, seed)` restated on the CPU (csrc/dense_common.h: two
    columns per 32-bit hash of (seed, row * width / 2 + column pair), kept where 16 hash bits >= round(p * 65536)), for
    seeds and sizes below 2^32 -- so the CPU suite checks the GPU cases' precondition under the very mask they run with."""
    assert 0 <= seed < 2 ** 32 and rows * (width // 2) < 2 ** 32 and width % 2 == 0
    idx = torch.arange(rows * (width // 2), dtype=torch.int64)
    h = _mix32(_mix32((idx ^ seed) & 0xFFFFFFFF))
    thr = int(p * 65536.0 + 0.5)
    keep = torch.stack([(h & 0xFFFF) >= thr, (h >> 16) >= thr], dim=1)
    return keep.reshape(rows, width)


def bernoulli_keep(rows: int, width: int, p: float, seed: int) -> torch.Tensor:
    return torch.rand(rows, width, generator=torch.Generator().manual_seed(seed)) >= p


def dropped(rows: torch.Tensor, keep: torch.Tensor, p: float) -> torch.Tensor:
    """fp32 (keep ? rows * scale32 : 0): what the forward and the weight gradient round."""
    rows = rows.detach().cpu().float()
    if keep is None:
        return rows
    return torch.where(keep, rows * torch.tensor(scale32(p), dtype=torch.float32), torch.zeros_like(rows))


def split(t, counts):
    return list(torch.split(t, list(counts)))


def case(h, m, counts, seed, n=N):
    """N(0, 1) states and incoming gradient, Xavier weights, random adjacency: (x [n, h], ws T x [m, h], adj, g [E, m])."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, generator=gen)
    ws = [C.xavier(m, h, gen) for _ in counts]
    adj = C.random_adjacency(n, counts, seed + 1)
    g = torch.randn(sum(counts), m, generator=gen)
    return x, ws, adj, g


def integer_case(h, m, counts, seed, n=N):
    """The ranges of C.integer_case: x in [-8, 8], W and g in [-2, 2], integers.  With p = 0.5 the scale is exactly 2, so
    every operand is an integer of magnitude <= 16, exact in bf16 and fp16, and every partial sum is far below 2^24."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (n, h), generator=gen).float()
    ws = [torch.randint(-2, 3, (m, h), generator=gen).float() for _ in counts]
    adj = C.random_adjacency(n, counts, seed + 1)
    g = torch.randint(-2, 3, (sum(counts), m), generator=gen).float()
    return x, ws, adj, g


def gathered(x, adj):
    return torch.cat([x.detach().cpu()[s.cpu()] for s, _ in adj]) if adj else x.new_zeros(0, x.shape[1])


def forward64(x, adj, ws, keep, p, dt=None):
    """msg[r] = rnd(keep ? x[src[r]] * scale : 0) rnd(W_t)^T in float64, type-major rows."""
    counts = [int(s.shape[0]) for s, _ in adj]
    rows = split(dropped(gathered(x, adj), keep, p), counts)
    return torch.cat([C.rnd64(r, dt) @ C.rnd64(w, dt).t() for r, w in zip(rows, ws)])


def forward32(x, adj, ws, keep, p, dt):
    """The same product by fp32 torch on the same rounded operands (for the floored bars of what sums over it)."""
    counts = [int(s.shape[0]) for s, _ in adj]
    rows = split(dropped(gathered(x, adj), keep, p), counts)
    return torch.cat([r.to(dt).float() @ w.detach().cpu().to(dt).float().t() for r, w in zip(rows, ws)])


def input_grad64(g, counts, ws, keep, p, dt=None):
    """out[r] = (rnd(g[r]) rnd(W_t)) * keep * scale in float64: [E, H]."""
    outs = [C.rnd64(gt, dt) @ C.rnd64(w, dt) for gt, w in zip(split(g.detach().cpu(), counts), ws)]
    out = torch.cat(outs)
    return out if keep is None else out * keep.double() * scale32(p)


def input_grad32(g, counts, ws, keep, p, dt):
    outs = [gt.to(dt).float() @ w.detach().cpu().to(dt).float() for gt, w in zip(split(g.detach().cpu(), counts), ws)]
    out = torch.cat(outs)
    return out if keep is None else out * keep.float() * torch.tensor(scale32(p), dtype=torch.float32)


def wgrad64(x, adj, g, keep, p, dt=None):
    """grad_w[t] = rnd(g_t)^T rnd(keep ? x[src_t] * scale : 0) in float64: [T, M, H]; a type without edges is zeros."""
    counts = [int(s.shape[0]) for s, _ in adj]
    rows = split(dropped(gathered(x, adj), keep, p), counts)
    return torch.stack([C.rnd64(gt, dt).t() @ C.rnd64(r, dt) for gt, r in zip(split(g.detach().cpu(), counts), rows)])


def wgrad32(x, adj, g, keep, p, dt):
    counts = [int(s.shape[0]) for s, _ in adj]
    rows = split(dropped(gathered(x, adj), keep, p), counts)
    return torch.stack([gt.to(dt).float().t() @ r.to(dt).float()
                        for gt, r in zip(split(g.detach().cpu(), counts), rows)])


def source_sum(per_edge, adj, n):
    """d_x = the per-edge input gradient summed onto its source rows."""
    src = torch.cat([s.cpu() for s, _ in adj])
    return torch.zeros(n, per_edge.shape[1], dtype=per_edge.dtype).index_add_(0, src, per_edge)


def references(x, ws, adj, g, keep, p, dt):
    """{what: (rounded float64, exact float64, bar)} for msg, g_in, d_w and d_x of one case: C.bar for the two per-row
    products, T.floored_bar for the two that sum over rows."""
    counts = [int(s.shape[0]) for s, _ in adj]
    n = x.shape[0]
    msg, msg_x = forward64(x, adj, ws, keep, p, dt), forward64(x, adj, ws, keep, p)
    gin, gin_x = input_grad64(g, counts, ws, keep, p, dt), input_grad64(g, counts, ws, keep, p)
    dw, dw_x = wgrad64(x, adj, g, keep, p, dt), wgrad64(x, adj, g, keep, p)
    dx, dx_x = source_sum(gin, adj, n), source_sum(gin_x, adj, n)
    dx32 = source_sum(input_grad32(g, counts, ws, keep, p, dt), adj, n)
    return {"msg": (msg, msg_x, C.bar(msg)), "g_in": (gin, gin_x, C.bar(gin)),
            "d_w": (dw, dw_x, T.floored_bar(dw, wgrad32(x, adj, g, keep, p, dt))),
            "d_x": (dx, dx_x, T.floored_bar(dx, dx32))}


def wgrad_counts(chunk: int):
    """Per-type edge counts of the weight-gradient cases: two chunks with a ragged last panel, an empty type, a single
    edge, and a type short of one panel."""
    return (chunk + 17, 0, 1, 40)


MIN_CHUNK = 512        # edges per partial of the 16-bit weight gradient at the tests' sizes (the kernel's floor)


def edge_case(h, m):
    """The random case of the forward / input-gradient / autograd-node tests at (H, M): COUNTS edges on N nodes.  (The
    seeds are ones at which the precondition holds under the mask of SEED: tests/test_edge_training_cpu.py checks it.)"""
    return case(h, m, COUNTS, 9110 + h + m)


def wgrad_case(h, m, chunk=MIN_CHUNK):
    return case(h, m, wgrad_counts(chunk), 9200 + h + m)
