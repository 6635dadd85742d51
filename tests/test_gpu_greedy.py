"""GruCopyingDecoder.greedy_decode on the MI355X: the step kernel (csrc/decode_step.hip) on crafted scores against the
float64 / float32 restatement of the reference's dict algorithm at every vocabulary size where it takes another path, the
module's device loop against the reference's fixtures (no vendor call, no host read-back inside the loop, the launches it
makes, the same bits twice), Graph2SeqModule.greedy_decode, and bf16 memories."""
import contextlib
import math
import types
from unittest import mock

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

import graph2seq_cases
from agg_paths import TOL, attributed_ok
from decoder_cases import build
from greedy_cases import (CASES, END_ID, MARGIN, START_ID, TOP_K, dict_step, inputs_of, load, restated_decode, state_of,
                          weights_from)
from ptgnn_amd import heads, ops, reduceops, sequence
from ptgnn_amd.gnn import GnnOutput

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
INF = math.inf
IDS = [name for name, _ in CASES]


def _refuse(name):
    def raiser(*args, **kwargs):
        raise AssertionError(f"{name} was called on the GPU route")
    return raiser


@contextlib.contextmanager
def no_vendor_calls():
    with mock.patch.object(nn.functional, "linear", _refuse("F.linear")), \
            mock.patch.object(nn.GRU, "forward", _refuse("nn.GRU.forward")), \
            mock.patch.object(nn.GRUCell, "forward", _refuse("nn.GRUCell.forward")), \
            mock.patch.object(torch, "topk", _refuse("torch.topk")), \
            mock.patch.object(torch, "sort", _refuse("torch.sort")), \
            mock.patch.object(torch, "unique", _refuse("torch.unique")):
        yield


class _Recorder(TorchDispatchMode):
    """(operator name, devices of its tensor results) of every operator that runs under it."""

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.ops.append((func.overloadpacket.__name__, [t.device.type for t in outs if isinstance(t, torch.Tensor)]))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step kernel on crafted scores
# ---------------------------------------------------------------------------------------------------------------------
def special_ids(V):
    return min(1, V - 1), min(3, V - 1)          # unk_id, end_id


def crafted(V, top_k, kinds, seed):
    """Raw scores [B, V], bias [V], copy scores [I], memory -> sample map (shuffled), element ids, the samples that are
    already done.  One sample per entry of `kinds`:
      none      no memories; its row's best entry is END
      one       one memory, its id the out-of-vocabulary key V + 3, its copy score far above the row: the next token is UNK
      same      300 memories that all carry one vocabulary id
      distinct  300 memories with 300 distinct ids, vocabulary ids and keys
      done      already done: two memories, nothing of its state may change
      edge      memories on the ids just inside and just outside the top K of its row (K < V), the key V + 3 again (the
                same key as `one`: the two must not merge) and some more
    Every row's entries outside its top K are moved down by 0.01, so the K-th and (K+1)-th largest are that far apart."""
    g = torch.Generator().manual_seed(seed)
    B, K = len(kinds), min(top_k, V)
    unk_id, end_id = special_ids(V)
    scores = torch.randn(B, V, generator=g) * 2.0
    bias = torch.randn(V, generator=g)
    for b in range(B):
        order = torch.sort(scores[b] + bias, descending=True, stable=True).indices
        scores[b, order[K:]] -= 0.01
    index, ids, copy = [], [], []
    for b, kind in enumerate(kinds):
        order = torch.sort(scores[b] + bias, descending=True, stable=True).indices
        if kind == "none":
            scores[b, end_id] = scores[b].max() + 3.0 - bias[end_id] + bias.max()
            continue
        if kind == "one":
            mine, c = [V + 3], torch.tensor([float(scores[b].max() + bias.max()) + 6.0])
        elif kind == "same":
            mine, c = [int(order[min(2, V - 1)])] * 300, torch.randn(300, generator=g)
        elif kind == "distinct":
            mine = (torch.randperm(V + 400, generator=g)[:300] if V >= 300 else torch.arange(300)).tolist()
            c = torch.randn(300, generator=g) * 2.0 + 2.0
        elif kind == "done":
            mine, c = [int(order[0]), V + 1], torch.randn(2, generator=g)
        else:
            mine = [V + 3, V + 3, int(order[0]), int(order[K - 1])] + ([int(order[K])] * 2 if K < V else []) \
                + torch.randint(0, V + 5, (9,), generator=g).tolist()
            c = torch.randn(len(mine), generator=g) + 1.0
        index += [b] * len(mine)
        ids += mine
        copy.append(c)
    index, ids = torch.tensor(index, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64)
    copy = torch.cat(copy) if copy else torch.zeros(0)
    shuffle = torch.randperm(index.shape[0], generator=g)                   # an unsorted origin index
    done = torch.tensor([kind == "done" for kind in kinds])
    return scores, bias, copy[shuffle], index[shuffle], ids[shuffle], done


def restated_step(scores, bias, copy, index, ids, top_k, dtype):
    """dict_step on the log-probabilities of the crafted scores in `dtype` (the joint normaliser of
    grucopydecoder.py:124-130)."""
    s = scores.to(dtype) + (bias.to(dtype) if bias is not None else 0)
    c = copy.to(dtype)
    B = s.shape[0]
    total = torch.full((B,), -INF, dtype=dtype)
    for b in range(B):
        if bool((index == b).any()):
            total[b] = torch.logsumexp(c[index == b], 0)
    norm = torch.logaddexp(torch.logsumexp(s, -1), total)
    return dict_step((s - norm.unsqueeze(1)).numpy(), (c - norm[index]).numpy(), index.numpy(), ids.numpy(), top_k), total


def run_step(scores, bias, copy, index, ids, done, top_k, step=1, T=3, tamper=lambda groups: groups):
    """ops.decode_step on the device -> the state after it and the state before it, as CPU tensors."""
    B, V = scores.shape
    unk_id, end_id = special_ids(V)
    _, total = restated_step(scores, bias, copy, index, ids, top_k, torch.float32)
    groups = tamper(ops.value_groups(index.to(DEV), ids.to(DEV), B, int(ids.max()) + 1 if ids.numel() else 1))
    state = [done.to(torch.int32), torch.where(done, 2, step), torch.where(done, -1.5, -0.25).float(),
             torch.full((B, T), -1, dtype=torch.int64), torch.full((B,), 7 % V, dtype=torch.int64)]
    state[3][:, :step] = 5 % V
    before = [t.clone() for t in state]
    state = [t.to(DEV) for t in state]
    count = ops.launch_counts(decode=True)
    ops.decode_step(scores.to(DEV), bias.to(DEV) if bias is not None else None, copy.to(DEV), total.to(DEV), groups, top_k,
                    unk_id, end_id, step, *state)
    assert ops.launches_since(count) == {"decode_step": 1}
    return [t.cpu() for t in state], before


def check_step(V, top_k, kinds, seed, with_bias=True):
    scores, bias, copy, index, ids, done = crafted(V, top_k, kinds, seed)
    if not with_bias:
        bias = None
    unk_id, end_id = special_ids(V)
    (got_done, got_len, got_lp, got_tok, got_next), before = run_step(scores, bias, copy, index, ids, done, top_k)
    again, _ = run_step(scores, bias, copy, index, ids, done, top_k)
    for a, b in zip((got_done, got_len, got_lp, got_tok, got_next), again):
        assert torch.equal(a, b)                                     # the same bits from run to run
    want64, _ = restated_step(scores, bias, copy, index, ids, top_k, torch.float64)
    want32, _ = restated_step(scores, bias, copy, index, ids, top_k, torch.float32)
    live = [b for b in range(len(kinds)) if not bool(done[b])]
    chosen = {}
    for b, kind in enumerate(kinds):
        if bool(done[b]):                                            # fed END, nothing else touched
            assert got_next[b] == end_id and got_done[b] == 1 and got_len[b] == before[1][b]
            assert got_lp[b] == before[2][b] and torch.equal(got_tok[b], before[3][b])
            continue
        predicted, value, gap, edge = want64[b]
        print(f"  V={V} K={top_k} {kind}: predicted {predicted} logprob {float(value):.6f} gap {gap:.3e} edge {edge:.3e}")
        assert gap >= MARGIN and edge >= MARGIN, (kind, gap, edge)    # the input condition: fp32 cannot flip the decision
        assert want32[b][0] == predicted
        chosen[b] = predicted
        assert got_next[b] == (predicted if predicted < V else unk_id), kind
        if predicted == end_id:
            assert got_done[b] == 1 and got_len[b] == before[1][b] and torch.equal(got_tok[b], before[3][b]), kind
        else:
            assert got_done[b] == 0 and got_len[b] == before[1][b] + 1 and got_tok[b, 1] == predicted, kind
            assert torch.equal(got_tok[b, [0, 2]], before[3][b, [0, 2]])
    got = got_lp[live] - before[2][live]                             # the step's own log-probabilities (a sum with -0.25)
    exact = torch.tensor([float(want64[b][1]) for b in live], dtype=torch.float64)
    ref32 = torch.tensor([float(want32[b][1]) for b in live], dtype=torch.float32)
    scale = max(1.0, float(exact.abs().max()))
    print(f"  V={V} K={top_k}: |got-fp32|={float((got - ref32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale:.3e}")
    assert attributed_ok(got, ref32, exact, TOL, scale)
    for b, kind in enumerate(kinds):                                  # what the crafted samples are there for
        if kind == "none":
            assert chosen[b] == end_id
        if kind == "one":
            assert chosen[b] == V + 3 and got_next[b] == unk_id
    return chosen


ALL_KINDS = ["distinct", "one", "none", "same", "done", "edge"]


@pytest.mark.parametrize("V", [1, 37, 100, 101, 257, 1000])
def test_step_kernel_against_the_restatement(V):
    check_step(V, 100, ALL_KINDS, seed=600 + V)


def test_step_kernel_on_a_long_row():
    check_step(20011, 100, ["distinct", "same", "edge"], seed=620)


@pytest.mark.parametrize("top_k", [1, 257])
def test_step_kernel_at_top_1_and_top_v(top_k):
    check_step(257, top_k, ALL_KINDS, seed=630 + top_k)


def test_step_kernel_without_a_bias():
    check_step(257, 100, ALL_KINDS, seed=640, with_bias=False)


def test_a_merge_inside_the_top_k_overturns_the_top_1_and_outside_it_does_not():
    """Two samples with the same row values and the same copy group on id g: in sample 0 the score of g is the K-th
    largest, in sample 1 the (K+1)-th (0.002 lower).  Merged with its vocabulary entry the group beats the row's top-1 by
    about 0.44; on its own (the merge starts from -inf) it loses by 0.3."""
    V, K, g, top1 = 257, 100, 41, 7
    values = torch.cat((-0.002 * torch.arange(K + 1).float(), -5.0 - 0.01 * torch.arange(V - K - 1).float()))
    others = [v for v in range(V) if v not in (g, top1)]
    scores = torch.empty(2, V)
    for b, rank in enumerate((K - 1, K)):
        order = [top1] + others[:rank - 1] + [g] + others[rank - 1:]
        scores[b, torch.tensor(order)] = values
    copy = torch.tensor([-0.3 - math.log(2.0)] * 4)                   # two memories per sample: a group of -0.3
    index, ids = torch.tensor([0, 1, 1, 0]), torch.tensor([g, g, g, g])
    done = torch.zeros(2, dtype=torch.bool)
    (got_done, got_len, got_lp, got_tok, got_next), before = run_step(scores, None, copy, index, ids, done, K)
    want, _ = restated_step(scores, None, copy, index, ids, K, torch.float64)
    assert [w[0] for w in want] == [g, top1] and min(w[2] for w in want) >= MARGIN and min(w[3] for w in want) >= MARGIN
    assert got_tok[:, 1].tolist() == [g, top1] and got_next.tolist() == [g, top1]
    exact = torch.tensor([float(w[1]) for w in want], dtype=torch.float64)
    assert float(((got_lp - before[2]).double() - exact).abs().max()) <= TOL
    assert float(exact[0] - exact[1]) > 0.4


def test_a_slot_outside_the_memories_is_clamped_counted_and_raised_later():
    from ptgnn_amd import _lib
    scores, bias, copy, index, ids, done = crafted(37, 100, ALL_KINDS, seed=650)
    ops.check_indices(DEV, sync=True)                                 # nothing pending

    def tamper(groups):
        rowptr, slot_memory, slot_ids = groups
        slot_memory = slot_memory.clone()
        slot_memory[0] = index.shape[0] + 7                           # read as memory 0
        slot_memory[1] = -2
        return rowptr, slot_memory, slot_ids
    state, _ = run_step(scores, bias, copy, index, ids, done, 100, tamper=tamper)
    assert bool(torch.isfinite(state[2]).all())
    with pytest.raises(_lib.PtgnnAmdError, match=r"2 node id\(s\) outside"):
        ops.check_indices(DEV, sync=True)
    ops.check_indices(DEV, sync=True)                                 # reported once


# ---------------------------------------------------------------------------------------------------------------------
# 2. the module's device loop against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------
def fixture_module(name, spec, dropout_rate=0.0):
    fx = load(name)
    module = build(spec, sequence, dropout_rate)
    module.load_state_dict(state_of(fx), strict=True)
    return fx, module.to(DEV).eval()


def decode(module, fx, spec, **changes):
    args = dict(inputs_of(fx, lambda t: t.to(DEV)), start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"], top_k=TOP_K)
    args.update(changes)
    return module.greedy_decode(**args)


@pytest.fixture(scope="module")
def exact_logprobs():
    """name -> the float64 restatement's log-probabilities: computed once, shared, left unchanged."""
    return {name: restated_decode(weights_from(load(name), torch.float64), inputs_of(load(name)), spec)[2]
            for name, spec in CASES}


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_module_decode_against_the_reference(name, spec, exact_logprobs):
    fx, module = fixture_module(name, spec, dropout_rate=0.2)        # eval(): dropout inactive
    T = spec["T"]
    marks, real = [], ops.decode_step
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_counts(aggregation=True, decode=True)
    with torch.cuda.stream(side), no_vendor_calls(), _Recorder() as rec:
        def spy(*args, **kwargs):
            marks.append(len(rec.ops))
            return real(*args, **kwargs)
        with mock.patch.object(ops, "decode_step", spy):
            tokens, lengths, logprobs = decode(module, fx, spec)
    ran = ops.launches_since(before)
    side.synchronize()
    assert ran.get("decode_step") == T and ran.get("segment_scores") == T and ran.get("attention_pool") == T, ran
    assert len(marks) == T
    inside = rec.ops[marks[0]:marks[-1]]                              # from the first step's launch to the last one's
    assert T == 1 or len(inside) > 5
    waits = [op for op, devices in inside
             if op in ("_local_scalar_dense", "item", "is_nonzero") or (op in ("_to_copy", "copy_") and "cpu" in devices)]
    assert not waits, waits
    assert tokens.is_cuda and tokens.dtype == torch.int64 and logprobs.dtype == torch.float32
    assert np.array_equal(tokens.cpu().numpy(), fx["token_ids"]) and np.array_equal(lengths.cpu().numpy(), fx["lengths"])
    exact = exact_logprobs[name]
    scale = max(1.0, float(np.abs(exact).max()))
    print(f"  {name}: |got - reference| = {float(np.abs(logprobs.cpu().double().numpy() - fx['logprobs']).max()):.3e} "
          f"|got - f64| = {float(np.abs(logprobs.cpu().double().numpy() - exact).max()):.3e} scale {scale:.3e}")
    assert attributed_ok(logprobs, torch.from_numpy(fx["logprobs"]), torch.from_numpy(exact), TOL, scale)
    for a, b in zip((tokens, lengths, logprobs), decode(module, fx, spec)):
        assert torch.equal(a, b)                                     # twice in a row, bit for bit
    ops.check_indices(DEV, sync=True)                                # nothing had to be clamped


def test_module_decode_edge_cases_and_errors():
    from ptgnn_amd import _lib
    name, spec = CASES[1]
    fx, module = fixture_module(name, spec, dropout_rate=0.2)
    before = ops.launch_counts(aggregation=True, decode=True)
    tokens, lengths, logprobs = decode(module, fx, spec, max_seq_len=0)
    inp = inputs_of(fx, lambda t: t.to(DEV))
    none = decode(module, fx, spec, initial_states=inp["initial_states"][:0], input_memories=inp["input_memories"][:0],
                  input_memories_origin_idx=inp["input_memories_origin_idx"][:0],
                  input_element_ids=inp["input_element_ids"][:0])
    assert ops.launches_since(before) == {}                           # empty results without a launch
    assert tokens.shape == (spec["B"], 0) and lengths.tolist() == [0] * spec["B"] and none[0].shape == (0, spec["T"])
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        decode(module, fx, spec, input_element_ids=inp["input_element_ids"] - 2000)
    with pytest.raises(_lib.PtgnnAmdError, match="dropout"):
        decode(module.train(), fx, spec)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Graph2SeqModule.greedy_decode
# ---------------------------------------------------------------------------------------------------------------------
def test_graph2seq_module_decodes_as_its_decoder_does_on_the_modules_own_memories():
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
    common = dict(input_element_ids=ids, start_id=START_ID, end_id=END_ID, max_seq_len=5)
    before = ops.launch_counts(aggregation=True, decode=True)
    got = module.greedy_decode(encoder_mb_data=encoder, **common)
    assert ops.launches_since(before).get("decode_step") == 5
    assert not any(p.grad is not None for p in module.parameters()) and not got[2].requires_grad
    with torch.no_grad():
        gnn_output = module._gnn(**encoder)
        memories = sequence._rows(gnn_output.output_node_representations, encoder["backbone_nodes"])
        want = module._decoder.greedy_decode(
            input_memories=memories, input_memories_origin_idx=encoder["backbone_graphs"],
            initial_states=module._get_initial_decoder_states(gnn_output), **common)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[0].shape == (spec["B"], 5) and int(got[1].max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. bf16 memories
# ---------------------------------------------------------------------------------------------------------------------
def test_bfloat16_memories_decode_to_the_tokens_of_the_fp32_route():
    """bf16 memories are up-cast on entry: the same bits as the fp32 route on the rounded memories.  On those memories the
    float64 restatement keeps every decision at least MARGIN = 1e-3 from flipping (asserted), and the tokens are its."""
    name, spec = CASES[3]
    fx, module = fixture_module(name, spec)
    x16 = inputs_of(fx)["input_memories"].bfloat16()
    want = restated_decode(weights_from(fx, torch.float64), dict(inputs_of(fx), input_memories=x16.double()), spec)
    print(f"  {name} on bf16-rounded memories: gap {want[3]:.3e} edge {want[4]:.3e}")
    assert want[3] >= MARGIN and want[4] >= MARGIN
    got16 = decode(module, fx, spec, input_memories=x16.to(DEV))
    got32 = decode(module, fx, spec, input_memories=x16.to(DEV).float())
    for a, b in zip(got16, got32):
        assert torch.equal(a, b)
    assert np.array_equal(got16[0].cpu().numpy(), want[0]) and np.array_equal(got16[1].cpu().numpy(), want[1])
