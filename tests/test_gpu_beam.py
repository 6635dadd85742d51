"""GruCopyingDecoder.beam_decode on the MI355X: the step kernel (csrc/beam_step.hip) on crafted inputs against the float64
/ float32 restatement of tests/beam_cases.py at every vocabulary size and width where it takes another path, the module's
device loop against the restatement on the cases of tests/test_beam_cpu.py (which asserts their input condition; no vendor
call, no host read-back inside the loop, the launches it makes, width 1 bit for bit greedy_decode),
Graph2SeqModule.beam_decode, and bf16 memories."""
import types
from unittest import mock

import numpy as np
import pytest
import torch

import graph2seq_cases
from agg_paths import TOL, attributed_ok
from beam_cases import WIDTHS_GPU, case, crafted_with_margin, restated_case
from decoder_cases import build
from greedy_cases import CASES, END_ID, MARGIN, START_ID, TOP_K
from ptgnn_amd import heads, ops, reduceops, sequence
from ptgnn_amd.gnn import GnnOutput
from test_gpu_greedy import _Recorder, no_vendor_calls

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
IDS = [name for name, _ in CASES]
ALL_KINDS = ["distinct", "one", "none", "same", "edge", "between", "finished"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step kernel on crafted inputs
# ---------------------------------------------------------------------------------------------------------------------
def run_step(inputs, total, top_k, W, step, T, tamper=lambda groups: groups):
    """ops.beam_step on the device -> (state out, next tokens, parent rows) and the state in, as CPU tensors."""
    scores, bias, copy, index, ids, beam, done = inputs
    B, V = beam.shape[0], scores.shape[1]
    unk_id, end_id = min(1, V - 1), min(3, V - 1)
    groups = tamper(ops.value_groups(index.to(DEV), ids.to(DEV), B, int(ids.max()) + 1 if ids.numel() else 1))
    tokens = torch.full((B, W, T), -1, dtype=torch.int64)
    for j in range(W):                                               # a history per slot that names it
        tokens[:, j, :step] = (7 + 3 * j + torch.arange(step)) % V
    lengths = torch.where(done, max(step - 1, 0), step)
    tokens[done] = torch.where(torch.arange(T) < max(step - 1, 0), tokens[done], -1)
    state_in = [beam.clone(), done.to(torch.int32), lengths, tokens]
    state_out = [torch.full_like(t, 77) for t in state_in]
    sent = [t.to(DEV) for t in (scores, copy, total)] + [bias.to(DEV) if bias is not None else None]
    dev_in, dev_out = [t.to(DEV) for t in state_in], [t.to(DEV) for t in state_out]
    next_tokens, parent_rows = (torch.full((B * W,), 77, dtype=torch.int64, device=DEV) for _ in range(2))
    count = ops.launch_counts(beam=True, decode=True, aggregation=True)
    ops.beam_step(sent[0], sent[3], sent[1], sent[2], groups, top_k, unk_id, end_id, step, dev_in, dev_out, next_tokens,
                  parent_rows)
    assert ops.launches_since(count) == {"beam_step": 1}
    for before, after in zip(state_in, dev_in):                      # what the step only reads is unchanged
        assert torch.equal(before, after.cpu())
    assert torch.equal(sent[0].cpu(), scores) and torch.equal(sent[1].cpu(), copy) and torch.equal(sent[2].cpu(), total)
    return [t.cpu() for t in dev_out] + [next_tokens.cpu(), parent_rows.cpu()], state_in


def check_step(V, top_k, W, kinds, seed, first_step=False):
    inputs, want64, want32, total, used, gap, edge = crafted_with_margin(V, top_k, W, kinds, seed, MARGIN, first_step)
    print(f"  V={V} K={top_k} W={W} seed {used}: decision gap {gap:.3e} top-K boundary gap {edge:.3e}")
    scores, bias, copy, index, ids, beam, done = inputs
    unk_id, end_id = min(1, V - 1), min(3, V - 1)
    step, T = (0, 3) if first_step else (2, 4)
    (got_beam, got_done, got_len, got_tok, got_next, got_parent), before = run_step(inputs, total, top_k, W, step, T)
    again, _ = run_step(inputs, total, top_k, W, step, T)
    for a, b in zip((got_beam, got_done, got_len, got_tok, got_next, got_parent), again):
        assert torch.equal(a, b)                                     # the same bits from run to run
    exact, ref32 = [], []
    for b, kind in enumerate(kinds):
        assert [(c[1], c[3]) for c in want32[b]] == [(c[1], c[3]) for c in want64[b]]
        for p, (score, parent, _, predicted) in enumerate(want64[b]):
            row = b * W + p
            assert int(got_parent[row]) == b * W + parent, (kind, p)  # the chosen (parent, id) pairs are exact
            exact.append(float(score))
            ref32.append(float(want32[b][p][0]))
            was_done = bool(done[b, parent])
            assert (predicted == -1) == was_done
            if was_done or predicted == end_id:
                assert got_done[b, p] == 1 and got_len[b, p] == before[2][b, parent], (kind, p)
                assert torch.equal(got_tok[b, p], before[3][b, parent]) and got_next[row] == end_id, (kind, p)
            else:
                assert got_done[b, p] == 0 and got_len[b, p] == before[2][b, parent] + 1, (kind, p)
                assert got_tok[b, p, step] == predicted and got_next[row] == (predicted if predicted < V else unk_id)
                rest = [c for c in range(T) if c != step]
                assert torch.equal(got_tok[b, p, rest], before[3][b, parent, rest]), (kind, p)
        chosen = [(c[1], c[3]) for c in want64[b]]
        if kind == "one" and not first_step:                          # the same key from every parent: distinct children
            assert chosen == [(j, V + 3) for j in range(W)] and got_next[b * W:(b + 1) * W].tolist() == [unk_id] * W
        if kind == "finished" and not first_step:
            assert sorted(chosen) == [(j, -1) for j in range(W)]
        if kind == "between" and W > 1 and not first_step:            # the finished slot between two live candidates
            assert chosen[1] == (1, -1) and chosen[0][1] != -1 and (W == 2 or chosen[2][1] != -1)
        if first_step:
            assert all(parent == 0 for parent, _ in chosen)            # the other slots are at -inf
        assert len(set(chosen)) == W                                  # a group on a best column replaces its entry
    got = got_beam.reshape(-1)
    exact, ref32 = torch.tensor(exact, dtype=torch.float64), torch.tensor(ref32, dtype=torch.float32)
    scale = max(1.0, float(exact.abs().max()))
    print(f"  V={V} K={top_k} W={W}: |got-fp32|={float((got - ref32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale:.3e}")
    assert attributed_ok(got, ref32, exact, TOL, scale)
    assert bool((got_beam[:, :-1] >= got_beam[:, 1:]).all())


@pytest.mark.parametrize("V,W", [(5, 1), (5, 2), (5, 3), (8, 8), (37, 1), (37, 2), (37, 3), (37, 8), (1000, 3), (1000, 8),
                                 (1025, 2), (1025, 8)])
def test_step_kernel_against_the_restatement(V, W):
    check_step(V, 100, W, ALL_KINDS, seed=700 + 10 * V + W)


def test_step_kernel_on_a_long_row():
    check_step(20000, 100, 8, ["distinct", "same", "edge", "between"], seed=720)


@pytest.mark.parametrize("V,W", [(37, 3), (37, 8), (1025, 8), (1025, 1)])
def test_step_kernel_where_the_wth_and_the_top_kth_thresholds_coincide(V, W):
    check_step(V, W, W, ALL_KINDS, seed=730 + V + W)


@pytest.mark.parametrize("V,W", [(37, 2), (1000, 8)])
def test_step_kernel_before_the_first_step(V, W):
    check_step(V, 100, W, ALL_KINDS, seed=740 + V + W, first_step=True)


def test_a_slot_outside_the_memories_is_clamped_counted_once_and_raised_later():
    from ptgnn_amd import _lib
    inputs, _, _, total, _, _, _ = crafted_with_margin(37, 100, 3, ALL_KINDS, 750, MARGIN)
    ops.check_indices(DEV, sync=True)                                 # nothing pending

    def tamper(groups):
        rowptr, slot_memory, slot_ids = groups
        slot_memory = slot_memory.clone()
        slot_memory[0] = inputs[3].shape[0] + 7                       # read as memory 0
        slot_memory[1] = -2
        return rowptr, slot_memory, slot_ids
    state, _ = run_step(inputs, total, 100, 3, 2, 4, tamper=tamper)
    assert bool(torch.isfinite(state[0]).all())
    with pytest.raises(_lib.PtgnnAmdError, match=r"2 node id\(s\) outside"):   # once, not once per slot of the beam
        ops.check_indices(DEV, sync=True)
    ops.check_indices(DEV, sync=True)                                 # reported once


def test_the_wrapper_refuses_widths_beyond_the_pool_and_shared_buffers():
    from ptgnn_amd import _lib
    groups = ops.value_groups(torch.zeros(1, dtype=torch.int64, device=DEV), torch.ones(1, dtype=torch.int64, device=DEV), 1, 2)

    def state(W):
        return [torch.zeros(1, W, device=DEV), torch.zeros(1, W, dtype=torch.int32, device=DEV),
                torch.zeros(1, W, dtype=torch.int64, device=DEV), torch.zeros(1, W, 2, dtype=torch.int64, device=DEV)]
    before = ops.launch_counts(beam=True)
    for W in (9, 12):
        with pytest.raises(_lib.PtgnnAmdError, match="head limit"):
            ops.beam_step(torch.zeros(W, 50, device=DEV), None, torch.zeros(1, W, device=DEV), torch.zeros(1, W, device=DEV),
                          groups, 100, 1, 3, 0, state(W), state(W), torch.zeros(W, dtype=torch.int64, device=DEV),
                          torch.zeros(W, dtype=torch.int64, device=DEV))
    shared = state(2)
    with pytest.raises(_lib.PtgnnAmdError, match="share"):
        ops.beam_step(torch.zeros(2, 50, device=DEV), None, torch.zeros(1, 2, device=DEV), torch.zeros(1, 2, device=DEV),
                      groups, 100, 1, 3, 0, shared, shared, torch.zeros(2, dtype=torch.int64, device=DEV),
                      torch.zeros(2, dtype=torch.int64, device=DEV))
    assert ops.launches_since(before) == {}


# ---------------------------------------------------------------------------------------------------------------------
# 2. the module's device loop against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def case_module(name, W, dropout_rate=0.0):
    spec, state, inputs = case(name, W)
    module = build(spec, sequence, dropout_rate)
    module.load_state_dict(state, strict=True)
    return spec, module.to(DEV).eval(), {k: v.to(DEV) for k, v in inputs.items()}


def decode(module, inputs, spec, W, **changes):
    args = dict(inputs, start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"], top_k=TOP_K, beam_width=W)
    args.update(changes)
    return module.beam_decode(**args)


@pytest.mark.parametrize("W", WIDTHS_GPU)
@pytest.mark.parametrize("name", IDS)
def test_module_beam_against_the_restatement(name, W):
    spec, module, inputs = case_module(name, W, dropout_rate=0.2)     # eval(): dropout inactive
    T = spec["T"]
    marks, real = [], ops.beam_step
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_counts(aggregation=True, decode=True, beam=True)
    with torch.cuda.stream(side), no_vendor_calls(), _Recorder() as rec:
        def spy(*args, **kwargs):
            marks.append(len(rec.ops))
            return real(*args, **kwargs)
        with mock.patch.object(ops, "beam_step", spy):
            tokens, lengths, logprobs = decode(module, inputs, spec, W)
    ran = ops.launches_since(before)
    side.synchronize()
    assert ran.get("beam_step") == T and ran.get("segment_scores") == T and ran.get("attention_pool") == T, ran
    assert "decode_step" not in ran and len(marks) == T
    inside = rec.ops[marks[0]:marks[-1]]                              # from the first step's launch to the last one's
    assert T == 1 or len(inside) > 5
    waits = [op for op, devices in inside
             if op in ("_local_scalar_dense", "item", "is_nonzero") or (op in ("_to_copy", "copy_") and "cpu" in devices)]
    assert not waits, waits
    assert tokens.is_cuda and tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and logprobs.dtype == torch.float32
    want = restated_case(name, W)
    assert np.array_equal(tokens.cpu().numpy(), want[0]) and np.array_equal(lengths.cpu().numpy(), want[1])
    exact, want32 = want[2], restated_case(name, W, torch.float32)[2]
    scale = max(1.0, float(np.abs(exact).max()))
    got = logprobs.cpu().double().numpy()
    print(f"  {name} W={W}: |got - fp32 restatement| = {float(np.abs(got - want32).max()):.3e} "
          f"|got - f64| = {float(np.abs(got - exact).max()):.3e} scale {scale:.3e}")
    assert attributed_ok(logprobs, torch.from_numpy(want32), torch.from_numpy(exact), TOL, scale)
    assert bool((logprobs[:, :-1] >= logprobs[:, 1:]).all())
    for a, b in zip((tokens, lengths, logprobs), decode(module, inputs, spec, W)):
        assert torch.equal(a, b)                                     # twice in a row, bit for bit
    if W == 1:                                                       # greedy decoding, bit for bit
        greedy = module.greedy_decode(**inputs, start_id=START_ID, end_id=END_ID, max_seq_len=T, top_k=TOP_K)
        assert torch.equal(tokens[:, 0], greedy[0]) and torch.equal(lengths[:, 0], greedy[1])
        assert torch.equal(logprobs[:, 0], greedy[2])
    ops.check_indices(DEV, sync=True)                                # nothing had to be clamped


def test_module_beam_edge_cases_and_errors():
    from ptgnn_amd import _lib
    name = IDS[1]
    spec, module, inp = case_module(name, 2, dropout_rate=0.2)
    before = ops.launch_counts(aggregation=True, decode=True, beam=True)
    tokens, lengths, logprobs = decode(module, inp, spec, 2, max_seq_len=0)
    none = decode(module, inp, spec, 2, initial_states=inp["initial_states"][:0], input_memories=inp["input_memories"][:0],
                  input_memories_origin_idx=inp["input_memories_origin_idx"][:0],
                  input_element_ids=inp["input_element_ids"][:0])
    assert ops.launches_since(before) == {}                           # empty results without a launch
    assert tokens.shape == (spec["B"], 2, 0) and lengths.tolist() == [[0, 0]] * spec["B"] and none[0].shape == (0, 2, spec["T"])
    with pytest.raises(_lib.PtgnnAmdError, match="head limit"):
        decode(module, inp, spec, 9)
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        decode(module, inp, spec, 2, input_element_ids=inp["input_element_ids"] - 2000)
    with pytest.raises(_lib.PtgnnAmdError, match="dropout"):
        decode(module.train(), inp, spec, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Graph2SeqModule.beam_decode, bf16 memories
# ---------------------------------------------------------------------------------------------------------------------
def test_graph2seq_module_searches_as_its_decoder_does_on_the_modules_own_memories():
    name, spec = graph2seq_cases.CASES[0]                             # the small stub-GNN case
    ns = types.SimpleNamespace(Graph2SeqModule=heads.Graph2SeqModule, GruCopyingDecoder=sequence.GruCopyingDecoder,
                               MultiheadSelfAttentionVarSizedElementReduce=reduceops.MultiheadSelfAttentionVarSizedElementReduce,
                               SimpleVarSizedElementReduce=reduceops.SimpleVarSizedElementReduce)
    torch.manual_seed(spec["seed"])
    module = graph2seq_cases.build(spec, ns, GnnOutput, dropout_rate=0.2).to(DEV).eval()
    inputs = graph2seq_cases.make_inputs(spec, torch.Generator().manual_seed(77))
    encoder = graph2seq_cases.call_args(spec, inputs, to=lambda t: t.to(DEV))["encoder_mb_data"]
    g = torch.Generator().manual_seed(78)
    n = inputs["backbone_nodes"].shape[0]
    ids = torch.where(torch.rand(n, generator=g) < 0.5, torch.randint(4, spec["V"], (n,), generator=g),
                      spec["V"] + torch.randint(0, 5, (n,), generator=g)).to(DEV)
    common = dict(input_element_ids=ids, start_id=START_ID, end_id=END_ID, max_seq_len=5, beam_width=3)
    before = ops.launch_counts(aggregation=True, decode=True, beam=True)
    got = module.beam_decode(encoder_mb_data=encoder, **common)
    assert ops.launches_since(before).get("beam_step") == 5
    assert not any(p.grad is not None for p in module.parameters()) and not got[2].requires_grad
    with torch.no_grad():
        gnn_output = module._gnn(**encoder)
        memories = sequence._rows(gnn_output.output_node_representations, encoder["backbone_nodes"])
        decoder_inputs = dict(input_memories=memories, input_memories_origin_idx=encoder["backbone_graphs"],
                              initial_states=module._get_initial_decoder_states(gnn_output))
        want = module._decoder.beam_decode(**decoder_inputs, **common)
        half = module._decoder.beam_decode(**dict(decoder_inputs, input_memories=memories.bfloat16()), **common)
        rounded = module._decoder.beam_decode(**dict(decoder_inputs, input_memories=memories.bfloat16().float()), **common)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    for a, b in zip(half, rounded):                                   # bf16 memories are up-cast on entry
        assert torch.equal(a, b)
    assert got[0].shape == (spec["B"], 3, 5) and int(got[1].max()) > 0
    assert bool((got[2][:, :-1] >= got[2][:, 1:]).all())
