"""The many-segment batches of tests/segment_batches.py have the properties the GPU tests rely on (checked without a GPU):
their element / chunk counts, which of the segments around the 64 / 1024 boundaries are empty, a chunk index that differs
from the segment index, an unsorted shuffled map -- and every float64 restatement is finite on the largest batch."""
import math
import time

import pytest
import torch

import segment_batches as SB

F64 = torch.float64


def test_the_2100_segment_batch_has_the_stated_counts():
    s = SB.sizes(2100, 0)
    assert len(s) == 2100 and sum(s) == 9033
    assert SB.chunk_count(s) == 1249
    assert sum(1 for c in s if c > 0) == 1215
    assert SB.chunk_count(s[:1024]) == 607                      # chunks in front of segment 1024: not its index
    assert {129, 128, 257} <= set(s) and {0, 1, 2, 3, 5} <= set(s)


def test_boundary_segments_are_empty_at_phase_0_and_two_are_not_at_phase_1():
    s0, s1 = SB.sizes(2100, 0), SB.sizes(2100, 1)
    assert [s0[i] for i in (0, 1, 63, 64, 1022, 1023)] == [0] * 6
    assert s1[64] > 0 and s1[1023] > 0


@pytest.mark.parametrize("G,phase", SB.CHUNK_BATCHES + SB.WINDOW_BATCHES)
def test_every_batch_mixes_empty_one_row_and_multi_chunk_segments(G, phase):
    s = SB.sizes(G, phase)
    assert len(s) == G and s[60] == 129 and all(c >= 0 for c in s)
    if phase == 0:
        assert s[0] == 0                                        # a leading empty segment; the trailing ones are added
    assert 0 in s and 1 in s
    runs = [i for i in range(1, G - 1) if s[i] == 0 and s[i - 1] == 0]
    assert runs and any(s[i + 1] > 0 for i in runs)             # runs of equal chunk-table entries in the middle
    if G > 121:
        assert s[121] == 128 and SB.chunk_count(s[:122]) == 3 + sum(1 for c in s[:122] if 0 < c < 128)
    if G > 182:
        assert s[182] == 257                                    # a three-chunk segment
    if G >= 1024:
        assert SB.chunk_count(s[:1024]) != 1024
    idx = SB.index_of(s + [0] * SB.TRAILING_EMPTY, False)
    assert idx.dtype == torch.int64 and idx.shape[0] == sum(s) and int(idx.max()) < G
    assert torch.equal(torch.bincount(idx, minlength=G + SB.TRAILING_EMPTY), torch.tensor(s + [0, 0]))
    assert bool((idx[1:] >= idx[:-1]).all())


@pytest.mark.parametrize("G,phase", SB.CHUNK_BATCHES + SB.WINDOW_BATCHES)
def test_a_shuffled_map_is_unsorted_and_holds_the_same_counts(G, phase):
    s = SB.sizes(G, phase)
    idx = SB.index_of(s, True, seed=G + phase)
    assert not bool((idx[1:] >= idx[:-1]).all())
    assert torch.equal(torch.bincount(idx, minlength=G), torch.tensor(s))
    assert torch.equal(idx, SB.index_of(s, True, seed=G + phase))          # seeded


def test_the_loops_leave_their_first_step_at_the_chosen_sizes():
    assert max(G for G, _ in SB.CHUNK_BATCHES) + SB.TRAILING_EMPTY > 2 * 1024       # three steps of SegmentScan<1024>
    assert {G for G, _ in SB.CHUNK_BATCHES} >= {65, 1024, 1025}
    assert all(G + SB.TRAILING_EMPTY > 256 for G, _ in SB.WINDOW_BATCHES + SB.CANDIDATE_BATCHES)
    assert [math.ceil(math.ceil(R / 128) / 256) for R in (32768, 32769, 70001)] == [1, 2, 3]
    assert [math.ceil((G + SB.TRAILING_EMPTY) / 256) for G, _ in SB.CANDIDATE_BATCHES] == [2, 3]


@pytest.mark.parametrize("G,phase", SB.CANDIDATE_BATCHES)
def test_candidate_batches_stay_small_and_skip_what_they_say(G, phase):
    x, w, cand_idx, slot_idx, cand_slot, correct, counts = SB.candidate_slots_batch(G, 64, seed=5)
    Cn = cand_idx.shape[0]
    assert len(counts) == G + SB.TRAILING_EMPTY and Cn == sum(counts) < 4000
    assert {63, 64, 65} <= set(counts) or G < 183
    assert not bool((cand_slot[1:] >= cand_slot[:-1]).all())
    assert cand_idx.unique().shape[0] == Cn
    inside = (correct >= 0) & (correct < Cn)
    assert int((~inside).sum()) == counts.count(0) + 1 and int((correct >= Cn).sum()) == 1
    assert bool((cand_slot[correct[inside]] == torch.nonzero(inside).flatten()).all())


def test_every_restatement_is_finite_in_float64_on_the_largest_batch():
    G, D, H, Lv = 2100 + SB.TRAILING_EMPTY, 64, 8, 5
    s = SB.sizes(2100, 0)
    idx = SB.index_of(s, True, seed=1)
    n = idx.shape[0]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, D, generator=g, dtype=F64)
    empty = torch.tensor([c == 0 for c in s] + [True] * SB.TRAILING_EMPTY)
    start = time.perf_counter()

    wk, wo = torch.randn(D, D, generator=g, dtype=F64) / 8.0, torch.randn(32, H * D, generator=g, dtype=F64) / 8.0
    y, scores = SB.ref_multihead(x, idx, G, wk, None, wo, H)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(scores).all()) and not bool(y[empty].any())

    out = SB.ref_weighted(x, idx, G, torch.randn(1, D, generator=g, dtype=F64) / 8.0)
    assert bool(torch.isfinite(out).all()) and not bool(out[empty].any())

    u = torch.randn(G, H, D, generator=g, dtype=F64) / 8.0
    pooled, top, lse = SB.ref_attention_pool(x, idx, G, u)
    assert bool(torch.isfinite(pooled).all()) and not bool(pooled[empty].any())
    assert torch.equal(lse == -SB.INF, empty.unsqueeze(1).expand(G, H)) and torch.equal(top == -SB.INF, lse == -SB.INF)

    v = torch.randn(G, Lv, D, generator=g, dtype=F64) / 8.0
    l = SB.segment_lse((v[idx] * x.unsqueeze(1)).sum(-1), idx, G)
    assert torch.equal(l == -SB.INF, empty.unsqueeze(1).expand(G, Lv)) and bool(torch.isfinite(l[~empty]).all())

    p = [0.5 + torch.rand(1, D, generator=g, dtype=F64) for _ in range(3)]
    assert bool(torch.isfinite(SB.ref_graphnorm(x, idx, *p, 1e-10)).all())
    means = SB.ref_graph_means(x, idx, G)
    assert bool(torch.isfinite(means).all()) and not bool(means[empty].any())

    counts = SB.sizes(600, 0) + [0] * SB.TRAILING_EMPTY
    kqv = torch.randn(sum(counts), 3 * 22, generator=g, dtype=F64)
    for max_nodes in (3, 40):
        offs = SB.window_offsets(counts, max_nodes)
        assert offs[-1] == sum(counts) and all(0 < b - a <= max_nodes for a, b in zip(offs[:-1], offs[1:]))
        att = SB.ref_attention(kqv, counts, max_nodes, 3, 6, 10)
        assert att.shape == (sum(counts), 30) and bool(torch.isfinite(att).all())

    R, C = 70001, 3
    logits = (torch.rand(R, C, generator=g) - 0.5) * 200.0
    loss, lse_rows, _ = SB.softmax_ref(logits, SB.softmax_targets(R, C, g), F64)
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(lse_rows).all())
    loss, _, _ = SB.sigmoid_ref(logits, torch.rand(R, C, generator=g) < 0.4, F64)
    assert math.isfinite(float(loss.detach()))

    xs, w, cand_idx, slot_idx, cand_slot, correct, counts = SB.candidate_slots_batch(700, D, seed=5)
    r = SB.candidate_ref(xs, w, cand_idx, slot_idx, cand_slot, correct, torch.randn(cand_idx.shape[0], generator=g),
                         torch.tensor(1.75), F64)
    none = torch.tensor([c == 0 for c in counts])
    assert math.isfinite(float(r[0].detach())) and torch.equal(r[2] == -SB.INF, none) and bool(torch.isfinite(r[1]).all())
    assert bool(torch.isfinite(r[4].grad).all()) and bool(torch.isfinite(r[5].grad).all())
    print(f"float64 restatements of the largest batches: {time.perf_counter() - start:.2f} s")
