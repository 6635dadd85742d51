"""The finishing route of GruCopyingDecoder.beam_decode on the MI355X: the step entry that writes back-pointers against
the entry that copies histories, chained over whole searches bit for bit, and the backtrack against those histories; crafted
steps under a table that differs between parents against the float64 / float32 restatement of tests/beam_finish_cases.py;
the module's device loop against the restatement on the triples tests/test_beam_finish_cpu.py vets (its launches, width 1
bit for bit greedy_decode); the early exit of beam_decode and greedy_decode (the number of steps issued is read off the
restatement's s*); and the index checks."""
import math

import numpy as np
import pytest
import torch

import beam_finish_cases as F
from agg_paths import TOL, attributed_ok
from beam_cases import crafted
from decoder_cases import build
from greedy_cases import END_ID, MARGIN, START_ID, TOP_K
from ptgnn_amd import _lib, ops, sequence

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
COMMON = dict(start_id=START_ID, end_id=END_ID, top_k=TOP_K)
FAMILIES = dict(aggregation=True, decode=True, beam=True, beam_finish=True)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def total_of(copy, index, B, W):
    """The copy scores' per-sample log-sum-exp [B, W] in float32, -inf for a sample without memories."""
    total = torch.full((B, W), -math.inf)
    for b in range(B):
        if bool((index == b).any()):
            total[b] = torch.logsumexp(copy[index == b], 0)
    return total


# ---------------------------------------------------------------------------------------------------------------------
# 1. the links entry against the old entry, chained; the backtrack against the copied histories
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 65])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_links_entry_and_backtrack_against_the_old_entry_over_a_whole_search(W, T):
    kinds, V = ["distinct", "between", "none"], 37
    B = len(kinds)
    scores, bias, copy, index, ids, beam, _ = crafted(V, 100, W, kinds, 800 + 10 * W + T, first_step=True)
    unk_id, end_id = 1, 3
    bias[end_id] += 1.5                                               # hypotheses do finish along the way
    total = total_of(copy, index, B, W).to(DEV)
    groups = ops.value_groups(index.to(DEV), ids.to(DEV), B, int(ids.max()) + 1)
    scores, bias, copy = scores.to(DEV), bias.to(DEV), copy.to(DEV)
    ones = torch.ones(T + 1, device=DEV)

    def start(with_tokens):
        state = [beam.to(DEV), torch.zeros(B, W, dtype=torch.int32, device=DEV),
                 torch.zeros(B, W, dtype=torch.int64, device=DEV)]
        return state + ([torch.full((B, W, T), -1, dtype=torch.int64, device=DEV)] if with_tokens else [])
    old, old_spare = start(True), [torch.full_like(t, 77) for t in start(True)]
    new, new_spare = start(False), [torch.full_like(t, 77) for t in start(False)]
    links = torch.full((T, B, W, 2), 77, dtype=torch.int32, device=DEV)
    live = torch.zeros(T, dtype=torch.int32, device=DEV)
    old_next, old_parent, new_next, new_parent = (torch.full((B * W,), 77, dtype=torch.int64, device=DEV) for _ in range(4))
    halfway, before = None, ops.launch_counts(**FAMILIES)
    for step in range(T):
        row_scores = torch.roll(scores, 5 * step, 1)                  # other scores every step, the same for both entries
        ops.beam_step(row_scores, bias, copy, total, groups, 100, unk_id, end_id, step, old, old_spare, old_next, old_parent)
        ops.beam_step_links(row_scores, bias, copy, total, groups, 100, unk_id, end_id, step, ones, new, new_spare, new_next,
                            new_parent, links, live)
        old, old_spare, new, new_spare = old_spare, old, new_spare, new
        assert same(old[:3], new) and torch.equal(old_next, new_next) and torch.equal(old_parent, new_parent), step
        assert int(live[step]) == int((new[1] == 0).sum())
        if step + 1 == (T + 1) // 2:
            halfway = old[3].clone()
    assert ops.launches_since(before) == {"beam_step": T, "beam_step_links": T}
    finished = int((new[1] != 0).sum())
    print(f"  W={W} T={T}: {finished} of {B * W} slots finished, lengths {new[2].min().item()} .. {new[2].max().item()}")
    tokens = torch.full((B, W, T), 77, dtype=torch.int64, device=DEV)  # every column is written
    ops.beam_backtrack(links, T, tokens)
    assert torch.equal(tokens, old[3])
    assert ((tokens >= 0).sum(-1) == new[2]).all()
    run = (T + 1) // 2                                                # steps_run < T: what the search held after `run` steps
    if run < T:
        # the slots after `run` steps are the final slots of a search that stopped there
        tokens.fill_(77)
        ops.beam_backtrack(links, run, tokens)
        assert torch.equal(tokens[:, :, :run], halfway[:, :, :run]) and bool((tokens[:, :, run:] == -1).all())
    tokens.fill_(77)
    ops.beam_backtrack(links, 0, tokens)
    assert bool((tokens == -1).all())
    assert ops.launches_since(before).get("beam_backtrack") == (3 if run < T else 2)


# ---------------------------------------------------------------------------------------------------------------------
# 2. crafted steps under a table that differs between the parents
# ---------------------------------------------------------------------------------------------------------------------
def run_links_step(inputs, lengths, scale, total, W, tamper=lambda groups: groups):
    scores, bias, copy, index, ids, beam, done = inputs
    B, V = beam.shape[0], scores.shape[1]
    unk_id, end_id = min(1, V - 1), min(3, V - 1)
    step, T = F.CRAFTED_STEP, F.CRAFTED_T
    groups = tamper(ops.value_groups(index.to(DEV), ids.to(DEV), B, int(ids.max()) + 1 if ids.numel() else 1))
    state_in = [beam.to(DEV), done.to(torch.int32).to(DEV), lengths.to(DEV)]
    kept = [t.clone() for t in state_in]
    state_out = [torch.full_like(t, 77) for t in state_in]
    next_tokens, parent_rows = (torch.full((B * W,), 77, dtype=torch.int64, device=DEV) for _ in range(2))
    links = torch.full((T, B, W, 2), 77, dtype=torch.int32, device=DEV)
    live = torch.zeros(T, dtype=torch.int32, device=DEV)
    before = ops.launch_counts(**FAMILIES)
    ops.beam_step_links(scores.to(DEV), bias.to(DEV), copy.to(DEV), total.to(DEV), groups, 100, unk_id, end_id, step,
                        scale.to(DEV), state_in, state_out, next_tokens, parent_rows, links, live)
    assert ops.launches_since(before) == {"beam_step_links": 1}
    assert same(kept, state_in)                                       # what the step only reads is unchanged
    other = torch.ones(T, dtype=torch.bool)
    other[step] = False
    assert bool((links[other] == 77).all()) and bool((live[other] == 0).all())
    return [t.cpu() for t in state_out] + [next_tokens.cpu(), parent_rows.cpu(), links[step].cpu(), int(live[step])]


@pytest.mark.parametrize("V,W", F.CRAFTED_SHAPES)
def test_crafted_steps_under_a_length_penalty(V, W):
    inputs, lengths, scale, want64, want32, plain, total, seed, gap, edge = F.crafted_case(V, W, MARGIN)
    print(f"  V={V} W={W} seed {seed}: key gap {gap:.3e} top-K boundary gap {edge:.3e}")
    done = inputs[6]
    unk_id, end_id = min(1, V - 1), min(3, V - 1)
    got_beam, got_done, got_len, got_next, got_parent, got_links, got_live = run_links_step(inputs, lengths, scale, total, W)
    again = run_links_step(inputs, lengths, scale, total, W)
    assert same((got_beam, got_done, got_len, got_next, got_parent, got_links), again[:6]) and again[6] == got_live
    exact, ref32, alive = [], [], 0
    for b in range(len(F.CRAFTED_KINDS)):
        for p, (score, parent, _, predicted, _) in enumerate(want64[b]):
            row = b * W + p
            assert int(got_parent[row]) == b * W + parent, (b, p)    # the chosen (parent, id) pairs are exact
            exact.append(float(score))
            ref32.append(float(want32[b][p][0]))
            was_done = bool(done[b, parent])
            assert (predicted == -1) == was_done
            if was_done or predicted == end_id:
                assert got_done[b, p] == 1 and got_len[b, p] == lengths[b, parent] and got_next[row] == end_id, (b, p)
                assert got_links[b, p].tolist() == [-1, parent], (b, p)
            else:
                alive += 1
                assert got_done[b, p] == 0 and got_len[b, p] == lengths[b, parent] + 1, (b, p)
                assert got_next[row] == (predicted if predicted < V else unk_id)
                assert got_links[b, p].tolist() == [predicted, parent], (b, p)
    assert got_live == alive and alive > 0
    got = got_beam.reshape(-1)
    exact, ref32 = torch.tensor(exact, dtype=torch.float64), torch.tensor(ref32, dtype=torch.float32)
    scale_of = max(1.0, float(exact.abs().max()))
    print(f"  V={V} W={W}: |got-fp32|={float((got - ref32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale_of:.3e}")
    assert attributed_ok(got, ref32, exact, TOL, scale_of)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the module's device loop against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def module_of(case, dropout_rate=0.0):
    spec, state, inputs = case
    module = build(spec, sequence, dropout_rate)
    module.load_state_dict(state, strict=True)
    return spec, module.to(DEV).eval(), {k: v.to(DEV) for k, v in inputs.items()}


@pytest.mark.parametrize("triple", F.TRIPLES_GPU, ids=lambda t: f"{t[0]}-w{t[1]}-a{t[2]}")
def test_module_finishing_route_against_the_restatement(triple):
    name, W, alpha = triple
    spec, module, inputs = module_of(F.case(*triple), dropout_rate=0.2)      # eval(): dropout inactive
    T = spec["T"]
    args = dict(inputs, max_seq_len=T, beam_width=W, **COMMON)
    before = ops.launch_counts(**FAMILIES)
    tokens, lengths, logprobs = module.beam_decode(**args, length_penalty=alpha)
    ran = ops.launches_since(before)
    assert ran.get("beam_step_links") == T and ran.get("beam_backtrack") == 1 and "beam_step" not in ran, ran
    assert "decode_step" not in ran and ran.get("segment_scores") == T and ran.get("attention_pool") == T, ran
    assert tokens.is_cuda and tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and logprobs.dtype == torch.float32
    want, want32 = F.restated_case(*triple), F.restated_case(*triple, torch.float32)
    assert np.array_equal(tokens.cpu().numpy(), want[0]) and np.array_equal(lengths.cpu().numpy(), want[1])
    scale = max(1.0, float(np.abs(want[2]).max()))
    got = logprobs.cpu().double().numpy()
    print(f"  {name} W={W} alpha={alpha}: |got - fp32 restatement| = {float(np.abs(got - want32[2]).max()):.3e} "
          f"|got - f64| = {float(np.abs(got - want[2]).max()):.3e} scale {scale:.3e}")
    assert attributed_ok(logprobs, torch.from_numpy(want32[2]), torch.from_numpy(want[2]), TOL, scale)
    assert same(module.beam_decode(**args, length_penalty=alpha), (tokens, lengths, logprobs))      # twice, bit for bit
    assert same(module.beam_decode(**args, length_penalty=alpha, early_exit=1), (tokens, lengths, logprobs))
    default = module.beam_decode(**args)                              # no penalty: the default call's bits
    before = ops.launch_counts(**FAMILIES)
    plain = module.beam_decode(**args, early_exit=T)
    ran = ops.launches_since(before)
    assert ran.get("beam_step_links") == T and ran.get("beam_backtrack") == 1 and "beam_step" not in ran, ran
    assert same(plain, default)
    if W == 1:                                                        # greedy decoding, bit for bit
        greedy = module.greedy_decode(**inputs, max_seq_len=T, **COMMON)
        assert same((plain[0][:, 0], plain[1][:, 0], plain[2][:, 0]), greedy)
    ops.check_indices(DEV, sync=True)                                 # nothing had to be clamped


# ---------------------------------------------------------------------------------------------------------------------
# 4. the early exit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", sorted(F.EARLY))
def test_early_exit_issues_the_steps_the_restatement_says_and_changes_no_bit(W):
    spec, module, inputs = module_of(F.early_case(W, False))
    T, s_star = spec["T"], F.restated_early(W, False)[3]              # read off the restatement
    assert s_star is not None and s_star < T - 2
    args = dict(inputs, max_seq_len=T, beam_width=W, **COMMON)
    before = ops.launch_counts(**FAMILIES)
    full = module.beam_decode(**args, early_exit=T)
    assert ops.launches_since(before).get("beam_step_links") == T
    want = F.restated_early(W, False)
    assert np.array_equal(full[0].cpu().numpy(), want[0]) and np.array_equal(full[1].cpu().numpy(), want[1])
    assert same(full, module.beam_decode(**args))
    for n in (1, 2):
        before = ops.launch_counts(**FAMILIES)
        got = module.beam_decode(**args, early_exit=n)
        ran = ops.launches_since(before)
        assert ran.get("beam_step_links") == min(T, s_star + n + 1) and ran.get("beam_backtrack") == 1, (n, ran)
        assert ran.get("attention_pool") == min(T, s_star + n + 1) and "beam_step" not in ran, (n, ran)
        assert same(got, full), n
        assert same(module.beam_decode(**args, early_exit=n, length_penalty=1.0),
                    module.beam_decode(**args, length_penalty=1.0))
    if W == 1:                                                        # greedy decoding's exit
        greedy_args = dict(inputs, max_seq_len=T, **COMMON)
        before = ops.launch_counts(**FAMILIES)
        whole = module.greedy_decode(**greedy_args)
        assert ops.launches_since(before).get("decode_step") == T
        assert same(whole, (full[0][:, 0], full[1][:, 0], full[2][:, 0]))
        for n in (1, 2, T):
            before = ops.launch_counts(**FAMILIES)
            got = module.greedy_decode(**greedy_args, early_exit=n)
            assert ops.launches_since(before).get("decode_step") == min(T, s_star + n + 1), n
            assert same(got, whole), n
    spec, module, inputs = module_of(F.early_case(W, True))           # one sample never ends: every step is issued
    assert F.restated_early(W, True)[3] is None
    args = dict(inputs, max_seq_len=T, beam_width=W, **COMMON)
    full = module.beam_decode(**args)
    for n in (1, 2):
        before = ops.launch_counts(**FAMILIES)
        got = module.beam_decode(**args, early_exit=n)
        assert ops.launches_since(before).get("beam_step_links") == T and same(got, full), n
    if W == 1:
        before = ops.launch_counts(**FAMILIES)
        got = module.greedy_decode(**dict(inputs, max_seq_len=T, **COMMON), early_exit=1)
        assert ops.launches_since(before).get("decode_step") == T
        assert same(got, (full[0][:, 0], full[1][:, 0], full[2][:, 0]))
    ops.check_indices(DEV, sync=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. checks
# ---------------------------------------------------------------------------------------------------------------------
def test_a_clamped_slot_is_counted_once_per_call_on_the_new_route():
    inputs, lengths, scale, _, _, _, total, _, _, _ = F.crafted_case(37, 3, MARGIN)
    ops.check_indices(DEV, sync=True)                                 # nothing pending

    def tamper(groups):
        rowptr, slot_memory, slot_ids = groups
        slot_memory = slot_memory.clone()
        slot_memory[0] = inputs[3].shape[0] + 7                       # read as memory 0
        slot_memory[1] = -2
        return rowptr, slot_memory, slot_ids
    state = run_links_step(inputs, lengths, scale, total, 3, tamper=tamper)
    assert bool(torch.isfinite(state[0]).all())
    with pytest.raises(_lib.PtgnnAmdError, match=r"2 node id\(s\) outside"):   # once, not once per slot of the beam
        ops.check_indices(DEV, sync=True)
    ops.check_indices(DEV, sync=True)                                 # reported once


def test_the_wrappers_refuse_what_the_entries_cannot_take():
    groups = ops.value_groups(torch.zeros(1, dtype=torch.int64, device=DEV), torch.ones(1, dtype=torch.int64, device=DEV),
                              1, 2)

    def state(W):
        return [torch.zeros(1, W, device=DEV), torch.zeros(1, W, dtype=torch.int32, device=DEV),
                torch.zeros(1, W, dtype=torch.int64, device=DEV)]

    def call(W, state_in, state_out, table=None, links=None, live=None):
        ops.beam_step_links(torch.zeros(W, 50, device=DEV), None, torch.zeros(1, W, device=DEV), torch.zeros(1, W, device=DEV),
                            groups, 100, 1, 3, 0, table if table is not None else torch.ones(3, device=DEV), state_in,
                            state_out, torch.zeros(W, dtype=torch.int64, device=DEV),
                            torch.zeros(W, dtype=torch.int64, device=DEV),
                            links if links is not None else torch.zeros(2, 1, W, 2, dtype=torch.int32, device=DEV), live)
    before = ops.launch_counts(**FAMILIES)
    with pytest.raises(_lib.PtgnnAmdError, match="head limit"):
        call(9, state(9), state(9))
    shared = state(2)
    with pytest.raises(_lib.PtgnnAmdError, match="share"):
        call(2, shared, shared)
    with pytest.raises(_lib.PtgnnAmdError, match="key_scale"):       # T + 1 entries
        call(2, state(2), state(2), table=torch.ones(2, device=DEV))
    with pytest.raises(_lib.PtgnnAmdError, match="live"):
        call(2, state(2), state(2), live=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.PtgnnAmdError, match="links"):
        call(2, state(2), state(2), links=torch.zeros(2, 1, 2, 2, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.PtgnnAmdError, match="steps_run"):
        ops.beam_backtrack(torch.zeros(2, 1, 2, 2, dtype=torch.int32, device=DEV), 3,
                           torch.zeros(1, 2, 2, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.PtgnnAmdError, match="tokens"):
        ops.beam_backtrack(torch.zeros(2, 1, 2, 2, dtype=torch.int32, device=DEV), 1,
                           torch.zeros(1, 2, 3, dtype=torch.int64, device=DEV))
    assert ops.launches_since(before) == {}
