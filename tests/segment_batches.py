"""Test support for the per-segment ops (the two pools, the segment scores, GraphNorm, the window table of block
attention, the two head merges): minibatches of MANY small segments, whose plans leave the first wave, the first step and
the first run of the one-workgroup loops that turn a plan into work, and the float64 / fp32 restatements the kernels are
compared with.  CPU only; never imported by the product package.

Where the loops stop being trivial (copied here; the code is the authority):
  * SegmentScan<1024> in k_pool_chunk_starts (csrc/weighted_pool.hip): wave sums from segment 65 on, `carry` from 1025 on
  * SegmentScan<256> in k_attention_windows (csrc/block_attention.hip): `carry` from graph 257 on
  * k_logit_merge / k_candidate_merge (csrc/task_heads.hip): 256 threads, thread t a run of ceil(n / 256) chunks of 128
    rows / slots -- runs of 2 from 32769 rows or 257 slots on
"""
import math

import torch
from torch import nn

CHUNK_ROWS = 128                      # csrc/segment_chunks.h kChunkRows
SMALL = (0, 0, 1, 3, 0, 2, 5)
BIG = (129, 128, 257)                 # one more than a chunk, a chunk, one more than two chunks
CANDIDATE_BIG = (63, 64, 65)          # around a wave: the candidate count stays in the low thousands
INF = float("inf")

# (segments with elements possible, phase); every call passes TRAILING_EMPTY further segments without elements
CHUNK_BATCHES = [(G, phase) for G in (65, 1024, 1025, 2100) for phase in (0, 1)]
WINDOW_BATCHES = [(257, 0), (600, 0)]
CANDIDATE_BATCHES = [(257, 0), (700, 0)]
TRAILING_EMPTY = 2


def sizes(G, phase, big=BIG):
    """Element counts of G segments: every 61st one long (cycling through `big`), the others 0 .. 5 by a period of 7."""
    return [big[(i // 61) % 3] if i % 61 == 60 else SMALL[(i + phase) % 7] for i in range(G)]


def chunk_count(counts):
    return sum(-(-c // CHUNK_ROWS) for c in counts)


def index_of(counts, shuffled, seed=0):
    """The int64 element -> segment map of segments with `counts` elements: sorted, or under a seeded permutation."""
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts, dtype=torch.int64))
    if shuffled:
        idx = idx[torch.randperm(idx.shape[0], generator=torch.Generator().manual_seed(seed))]
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# the pools (tests/test_gpu_attention_pool.py)
# ---------------------------------------------------------------------------------------------------------------------
def ref_multihead(x, idx, G, wk, wv, wo, H):
    """varsizedsummary.py:140-178 with a `max` query (hidden = D), any dtype / device."""
    n, D = x.shape
    q = torch.zeros(G, D, dtype=x.dtype, device=x.device).scatter_reduce(0, idx.unsqueeze(1).expand(-1, D), x, "amax",
                                                                         include_self=False)
    keys = (x @ wk.t()).reshape(n, H, -1)
    scores = (q[idx].reshape(n, H, -1) * keys).sum(-1) / math.sqrt(keys.shape[-1])
    top = torch.full((G, H), float("-inf"), dtype=x.dtype, device=x.device).scatter_reduce(
        0, idx.unsqueeze(1).expand(-1, H), scores.detach(), "amax")
    e = (scores - top[idx]).exp()
    total = torch.zeros(G, H, dtype=x.dtype, device=x.device).index_add(0, idx, e)
    p = e / total[idx]
    vals = (x @ wv.t()).reshape(n, H, -1) if wv is not None else x.unsqueeze(1)
    rows = (p.unsqueeze(-1) * vals).reshape(n, -1)
    per = torch.zeros(G, rows.shape[1], dtype=x.dtype, device=x.device).index_add(0, idx, rows)
    return per @ wo.t(), scores


def ref_weighted(x, idx, G, w):
    """varsizedsummary.py:68-81: sigmoid(Linear(D, 1)) scores, the scaled rows summed per sample; any dtype / device."""
    score = 1.0 / (1.0 + torch.exp(-(x @ w.t()).squeeze(-1)))
    return torch.zeros(G, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, idx, x * score.unsqueeze(-1))


def segment_lse(scores, index, n):
    """Per-segment log-sum-exp of scores [E, L] over n segments; -inf for a segment without elements."""
    top = torch.full((n, scores.shape[1]), -INF, dtype=scores.dtype, device=scores.device).scatter_reduce(
        0, index.unsqueeze(1).expand_as(scores), scores.detach(), "amax")
    safe = torch.where(top == -INF, torch.zeros_like(top), top)
    total = torch.zeros_like(top).index_add(0, index, (scores - safe[index]).exp())
    return torch.where(top == -INF, top, total.log() + safe)


def ref_attention_pool(x, idx, G, u):
    """The op under the multi-head reducer (ops.attention_pool): s[i, h] = u[g(i), h] . x_i, a softmax of s[., h] within
    each segment, P[g, h] = sum_i p[i, h] x_i.  Returns (P [G, H, D], top [G, H], lse [G, H]); top and lse are -inf for a
    segment without elements (the kernel writes 0 there)."""
    H = u.shape[1]
    s = (u[idx] * x.unsqueeze(1)).sum(-1)                                          # [n, H]
    top = torch.full((G, H), -INF, dtype=x.dtype, device=x.device).scatter_reduce(
        0, idx.unsqueeze(1).expand(-1, H), s.detach(), "amax")
    lse = segment_lse(s, idx, G)
    p = (s - lse[idx]).exp()
    pooled = torch.zeros(G, H, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, idx, p.unsqueeze(-1) * x.unsqueeze(1))
    return pooled, top, lse


# ---------------------------------------------------------------------------------------------------------------------
# GraphNorm (tests/test_gpu_graphnorm.py)
# ---------------------------------------------------------------------------------------------------------------------
def ref_graphnorm(x, idx, gamma, alpha, bias, eps):
    """graphnorm.py:36-46 (scatter_mean = index_add / max(count, 1)), any dtype / device."""
    D, n_graphs = x.shape[1], int(idx.max()) + 1
    count = torch.zeros(n_graphs, dtype=x.dtype, device=x.device).index_add_(
        0, idx, torch.ones(idx.shape[0], dtype=x.dtype, device=x.device)).clamp(min=1).unsqueeze(1)

    def scatter_mean(v):
        return torch.zeros(n_graphs, D, dtype=x.dtype, device=x.device).index_add(0, idx, v) / count

    per_graph_mean = scatter_mean(x)
    shifted = x - alpha * per_graph_mean[idx]
    sigma_2 = scatter_mean(torch.pow(shifted, 2)) + eps
    return gamma * shifted / torch.sqrt(sigma_2[idx]) + bias


def ref_graph_means(x, idx, G):
    """The per-graph means [G, D] GraphNorm's forward hands to its backward; 0 for a graph without nodes."""
    count = torch.zeros(G, dtype=x.dtype, device=x.device).index_add_(
        0, idx, torch.ones(idx.shape[0], dtype=x.dtype, device=x.device)).clamp(min=1).unsqueeze(1)
    return torch.zeros(G, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, idx, x) / count


# ---------------------------------------------------------------------------------------------------------------------
# block attention (tests/test_gpu_selfatt.py): selfattmessagepassing.py:104-117 with a padded mask
# ---------------------------------------------------------------------------------------------------------------------
def window_offsets(counts, max_num_nodes):
    offs, first = [], 0
    for c in counts:
        offs += [first + lo for lo in range(0, c, max_num_nodes)]
        first += c
    return offs + [first]


def ref_attention(kqv, counts, max_num_nodes, heads, dk, dv, mask=None):
    """out [N, heads dv] in the dtype of kqv; `mask` [N heads, W]: the dropout multiplier of (row r heads + h, column j)."""
    n = kqv.shape[0]
    offs = window_offsets(counts, max_num_nodes)
    lens = torch.tensor([b - a for a, b in zip(offs[:-1], offs[1:])])
    W, Lmax = lens.shape[0], int(lens.max())
    pos = torch.arange(Lmax)
    valid = pos[None, :] < lens[:, None]                                           # [W, L]
    rows = (torch.tensor(offs[:-1])[:, None] + pos[None, :]).clamp(max=n - 1)      # [W, L]
    x = kqv.reshape(n, heads, 2 * dk + dv)[rows]                                   # [W, L, heads, :]
    keys, queries, values = x[..., :dk], x[..., dk:2 * dk], x[..., 2 * dk:]
    scores = torch.einsum("wkhd,wvhd->wkhv", keys, queries) / dk ** 0.5
    scores = scores.masked_fill(~valid[:, None, None, :], float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    if mask is not None:
        m = mask.reshape(n, heads, -1)[rows][..., :Lmax]                          # [W, L(k), heads, L(v)]
        probs = probs * m.to(probs.dtype)
    out = torch.einsum("wkhv,wvhd->wkhd", probs, values)                           # [W, L, heads, dv]
    return out[valid].reshape(n, heads * dv)


# ---------------------------------------------------------------------------------------------------------------------
# the task heads (tests/test_gpu_heads.py)
# ---------------------------------------------------------------------------------------------------------------------
def softmax_ref(logits, targets, dtype):
    """(loss, lse, per-row loss) of the softmax mode in `dtype`: rows whose target is outside [0, C) are ignored."""
    l = logits.detach().to(dtype).requires_grad_(True)
    C = l.shape[1]
    lse = torch.logsumexp(l, dim=-1)
    live = (targets >= 0) & (targets < C)
    picked = l.gather(1, targets.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    rows = torch.where(live, lse - picked, torch.zeros_like(lse))
    return rows.sum() / live.sum(), lse, l


def sigmoid_ref(logits, targets, dtype):
    l = logits.detach().to(dtype).requires_grad_(True)
    t = targets.to(dtype)
    # ppi.py:59-62 itself: max(l, 0) - l t + log1p(exp(-|l|)) with the analytic gradient sigmoid(l) - t (spelled with clamp
    # and abs, autograd takes a subgradient at a logit that is exactly 0 -- 1 - t instead of 0.5 - t)
    rows = nn.functional.binary_cross_entropy_with_logits(l, t, reduction="none").sum(-1)
    return rows.mean(), None, l


def softmax_targets(R, C, gen):
    t = torch.randint(0, C, (R,), generator=gen)
    t[0], t[R - 1] = 0, C - 1
    if R >= 3:
        t[1] = -100                   # nn.CrossEntropyLoss's ignore_index
    if R >= 4:
        t[2] = C                      # the reference device-asserts; skipped and counted here
    return t


def candidate_ref(x, w, cand_idx, slot_idx, cand_slot, correct, cot, g, dtype):
    """(loss, scores, lse, argmax, x, w) in `dtype`; the backward of g * loss + sum(cot * scores) has run."""
    x = x.detach().to(dtype).requires_grad_(True)
    w = w.detach().to(dtype).requires_grad_(True)
    D, G, Cn = x.shape[1], slot_idx.shape[0], cand_idx.shape[0]
    scores = x[cand_idx] @ w[0, :D] + (x[slot_idx] @ w[0, D:])[cand_slot]
    top = torch.full((G,), -INF, dtype=dtype, device=x.device).scatter_reduce(0, cand_slot, scores.detach(), "amax")
    safe = torch.where(top == -INF, torch.zeros_like(top), top)
    total = torch.zeros(G, dtype=dtype, device=x.device).index_add(0, cand_slot, (scores - safe[cand_slot]).exp())
    lse = torch.where(top == -INF, top, total.log() + safe)
    position = torch.arange(Cn, device=x.device)
    best = torch.where(scores.detach() == top[cand_slot], position, torch.full_like(position, Cn))
    argmax = torch.full((G,), Cn, dtype=torch.int64, device=x.device).scatter_reduce(0, cand_slot, best, "amin")
    ok = (correct >= 0) & (correct < Cn)
    ok = ok & (cand_slot[correct.clamp(0, Cn - 1)] == torch.arange(G, device=x.device))
    terms = torch.where(ok, scores[correct.clamp(0, Cn - 1)] - torch.where(ok, lse, torch.zeros_like(lse)),
                        torch.zeros_like(lse))
    loss = -terms.sum() / G
    (loss * g.to(dtype) + (scores * cot.to(dtype)).sum()).backward()
    return loss, scores, lse, argmax, x, w


def candidate_slots_batch(G, D, seed, num_nodes=4000):
    """A VarMisuse minibatch over G + TRAILING_EMPTY slots with sizes(G, 0, CANDIDATE_BIG) candidates: an unsorted candidate
    -> slot map, distinct candidate nodes, per slot the position of its middle candidate as the correct one -- -1 for an
    empty slot and, for the LAST non-empty slot, an index past the end (both skipped and counted).
    Returns (x, w, cand_idx, slot_idx, cand_slot, correct, counts)."""
    gen = torch.Generator().manual_seed(seed)
    counts = sizes(G, 0, CANDIDATE_BIG) + [0] * TRAILING_EMPTY
    slots, Cn = len(counts), sum(counts)
    assert Cn <= num_nodes
    cand_slot = index_of(counts, True, seed + 1)
    cand_idx = torch.randperm(num_nodes, generator=gen)[:Cn]
    slot_idx = torch.randint(0, num_nodes, (slots,), generator=gen)
    order = torch.argsort(cand_slot, stable=True)                  # the candidates of a slot, in candidate order
    first = [0]
    for c in counts:
        first.append(first[-1] + c)
    correct = torch.tensor([-1 if c == 0 else int(order[first[s] + c // 2]) for s, c in enumerate(counts)])
    correct[max(s for s, c in enumerate(counts) if c > 0)] = Cn + 7
    x = torch.randn(num_nodes, D, generator=gen)
    w = torch.randn(1, 2 * D, generator=gen) / math.sqrt(D)
    return x, w, cand_idx, slot_idx, cand_slot, correct, counts
