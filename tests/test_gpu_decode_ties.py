"""The decoding-step kernels (csrc/decode_step.hip, csrc/beam_step.hip, csrc/decode_common.h) on the MI355X where their
decisions rest on exact ties and on the edge rows of the radix select: the cases of tests/tie_cases.py (checked on the CPU
by tests/test_decode_ties_cpu.py) against the unchanged restatements of tests/greedy_cases.py and tests/beam_cases.py, one
launch per case through run_step of tests/test_gpu_greedy.py / tests/test_gpu_beam.py (which assert the one launch).

What the cases catch: each of these one-line changes of the library, built with scripts/build_variant.sh and run once on
the MI355X, failed the cases named and no others.
  `c <= cut` -> `c < cut` in the group admission of decode_step.hip: greedy small_runs, blocks, all_equal, all_equal_bias,
      v_is_k_plus_1, zeros, masked (every greedy case with a probe on the last admitted column of a run);
  `before == need - 1` -> `before == need` in the tie scan of RadixSelect::select: the same greedy cases and the beam cases
      v37_*, v1025_k100_w8, v2500_*, keys_w3, edges_v9_*, edges_v2500_*;
  order_key without its `v == 0.0f` fold: greedy zeros, beam keys_w3;
  `c.id < best.id` -> `c.id > best.id` in the top-1 merge of decode_step.hip: greedy top1_v1024, top1_v1025, top1_v2049,
      all_equal, all_equal_bias;
  `p < parent` -> `p > parent` in k_beam_select: beam v37_*, v1025_k100_w8, v2500_*, edges_*;
  the `a.id < b.id` leg dropped from before() in beam_step.hip: the same beam cases and keys_w3."""
import pytest
import torch

import test_gpu_beam as beam_gpu
import test_gpu_greedy as greedy_gpu
from agg_paths import TOL, attributed_ok
from greedy_cases import MARGIN  # noqa: F401  (the margin of tie_cases' input condition; tests/test_decode_ties_cpu.py compares)
from tie_cases import BEAM, GREEDY, case

pytestmark = pytest.mark.gpu

GREEDY_NAMES = list(GREEDY)
BEAM_NAMES = list(BEAM)


def _attributed(got, want64, want32, what):
    exact = torch.tensor([float(v) for v in want64], dtype=torch.float64)
    ref32 = torch.tensor([float(v) for v in want32], dtype=torch.float32)
    scale = max(1.0, float(exact.abs().max()))
    print(f"  {what}: |got-fp32|={float((got - ref32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale:.3e}")
    assert attributed_ok(got, ref32, exact, TOL, scale)


@pytest.mark.filterwarnings("ignore:invalid value encountered")     # -inf - -inf in dict_step's gaps, which nothing reads
@pytest.mark.parametrize("name", GREEDY_NAMES)
def test_greedy_step_on_exact_ties_and_edge_rows(name):
    inputs, top_k, _, notes, want64, want32, _, _ = case("greedy", name)
    V = inputs[0].shape[1]
    unk_id, end_id = greedy_gpu.special_ids(V)
    (got_done, got_len, got_lp, got_tok, got_next), before = greedy_gpu.run_step(*inputs, top_k)
    again, _ = greedy_gpu.run_step(*inputs, top_k)
    for a, b in zip((got_done, got_len, got_lp, got_tok, got_next), again):
        assert torch.equal(a, b)                                     # the same bits from run to run
    for b, note in enumerate(notes):
        predicted = want64[b][0]
        assert want32[b][0] == predicted
        print(f"  {name} {note['family']}: predicted {predicted} logprob {float(want64[b][1]):.6f}")
        assert got_next[b] == (predicted if predicted < V else unk_id), (note["family"], b)
        if predicted == end_id:
            assert got_done[b] == 1 and got_len[b] == before[1][b] and torch.equal(got_tok[b], before[3][b]), b
        else:
            assert got_done[b] == 0 and got_len[b] == before[1][b] + 1 and got_tok[b, 1] == predicted, (note["family"], b)
            assert torch.equal(got_tok[b, [0, 2]], before[3][b, [0, 2]])
        if "expect" in note:
            assert predicted == note["expect"]
    _attributed(got_lp - before[2], [w[1] for w in want64], [w[1] for w in want32], name)


@pytest.mark.parametrize("name", BEAM_NAMES)
def test_beam_step_on_exact_ties_and_edge_rows(name):
    inputs, top_k, W, notes, want64, want32, total, _ = case("beam", name)
    done = inputs[6]
    V = inputs[0].shape[1]
    unk_id, end_id = min(1, V - 1), min(3, V - 1)
    step, T = 2, 4
    (got_beam, got_done, got_len, got_tok, got_next, got_parent), before = beam_gpu.run_step(inputs, total, top_k, W, step, T)
    again, _ = beam_gpu.run_step(inputs, total, top_k, W, step, T)
    for a, b in zip((got_beam, got_done, got_len, got_tok, got_next, got_parent), again):
        assert torch.equal(a, b)                                     # the same bits from run to run
    assert not bool(done.any())
    exact, ref32 = [], []
    for b, note in enumerate(notes):
        assert [(c[1], c[3]) for c in want32[b]] == [(c[1], c[3]) for c in want64[b]]
        print(f"  {name} {note['family']}: {[(c[1], c[2], c[3]) for c in want64[b]]}")
        for p, (score, parent, _, predicted) in enumerate(want64[b]):
            row = b * W + p
            assert int(got_parent[row]) == b * W + parent, (note["family"], b, p)
            exact.append(score)
            ref32.append(want32[b][p][0])
            if predicted == end_id:
                assert got_done[b, p] == 1 and got_len[b, p] == before[2][b, parent], (note["family"], b, p)
                assert torch.equal(got_tok[b, p], before[3][b, parent]) and got_next[row] == end_id, (note["family"], b, p)
            else:
                assert got_done[b, p] == 0 and got_len[b, p] == before[2][b, parent] + 1, (note["family"], b, p)
                assert got_tok[b, p, step] == predicted, (note["family"], b, p)
                assert got_next[row] == (predicted if predicted < V else unk_id), (note["family"], b, p)
                rest = [c for c in range(T) if c != step]
                assert torch.equal(got_tok[b, p, rest], before[3][b, parent, rest]), (note["family"], b, p)
        chosen = [(c[1], c[3]) for c in want64[b]]
        assert len(set(chosen)) == W                                  # a group on a best column replaces its entry
        if "expect" in note:
            assert chosen == note["expect"]
    _attributed(got_beam.reshape(-1), exact, ref32, name)
    assert bool((got_beam[:, :-1] >= got_beam[:, 1:]).all())
