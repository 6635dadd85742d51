"""The finishing route of GruCopyingDecoder.beam_decode (length_penalty, early_exit) and greedy_decode's early exit
without a GPU: the input condition of every (case, width, penalty) triple, crafted step and early-exit case the CPU and GPU
tests use (every decision at least MARGIN from flipping in float64, in key units; the penalty does reorder something), the
CPU route against the float64 / float32 restatement of tests/beam_finish_cases.py, bit equality with the default call,
argument errors, Graph2SeqModule, and the C ABI of the new entries as far as it goes without a device."""
import ctypes
import inspect
import math
import os
import re
import types
from unittest import mock

import numpy as np
import pytest
import torch

import beam_cases
import beam_finish_cases as F
from agg_paths import TOL, attributed_ok
from decoder_cases import build
from greedy_cases import END_ID, MARGIN, START_ID, TOP_K
from ptgnn_amd import _lib, heads, ops, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = dict(start_id=START_ID, end_id=END_ID, top_k=TOP_K)
TRIPLES = sorted(set(F.TRIPLES_CPU) | set(F.TRIPLES_GPU))
SYMBOLS = sorted(["ptgnn_amd_search_step_links_f32", "ptgnn_amd_search_backtrack", "ptgnn_amd_greedy_step_live_f32"])


def triple_id(t):
    return f"{t[0]}-w{t[1]}-a{t[2]}"


def module_of(case, dropout_rate=0.0):
    spec, state, inputs = case
    module = build(spec, sequence, dropout_rate).eval()
    module.load_state_dict(state, strict=True)
    return spec, module, inputs


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# input conditions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", TRIPLES, ids=triple_id)
def test_every_decision_of_a_triple_is_a_margin_away_from_flipping_in_key_units(triple):
    name, W, alpha = triple
    spec, state, inputs = F.case(*triple)
    tokens, lengths, sums, s_star, gap, edge = F.restated_case(*triple)
    print(f"  {name} W={W} alpha={alpha} (seed {F.SEEDED.get(triple)}): key gap {gap:.3e}, top-K boundary gap {edge:.3e}, "
          f"s* {s_star}")
    assert gap >= MARGIN and edge >= MARGIN                           # no sample, no step is left out of either minimum
    assert tokens.shape == (spec["B"], W, spec["T"]) and not np.isnan(sums).any()
    low = F.restated_case(*triple, torch.float32)                     # fp32 takes the same decisions
    assert np.array_equal(low[0], tokens) and np.array_equal(low[1], lengths) and low[3] == s_star


@pytest.mark.parametrize("name,W", [("greedy_b5_v37_t4", 3), ("greedy_b5_v1000_t8", 2), ("greedy_b1_v37_t1", 12)])
def test_the_restatement_with_an_all_ones_table_is_the_restatement_of_the_default_search(name, W):
    spec, state, inputs = beam_cases.case(name, W)
    for dtype in (torch.float64, torch.float32):
        got = F.restated_finish(F.weights_of_state(state, dtype), inputs, spec["T"], W, 0.0)
        want = beam_cases.restated_case(name, W, dtype)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[4] >= want[3] and got[5] >= want[4]                # its gaps: those of the steps with something live
    assert bool((F.scale_table(0.0, 9) == 1.0).all())


def test_the_penalty_reorders_a_module_case_and_a_crafted_step():
    name, W, alpha = F.REORDERED
    assert W >= 2 and F.REORDERED in F.TRIPLES_CPU and F.REORDERED not in F.SEEDED
    keyed, plain = F.restated_case(name, W, alpha), beam_cases.restated_case(name, W)
    differ = [b for b in range(keyed[0].shape[0]) if not np.array_equal(keyed[0][b, 0], plain[0][b, 0])]
    print(f"  {name} W={W} alpha={alpha}: slot 0 differs from the unnormalised search for samples {differ}")
    assert differ
    reordered = []
    for V, W in F.CRAFTED_SHAPES:
        inputs, lengths, scale, want64, want32, plain, total, seed, gap, edge = F.crafted_case(V, W, MARGIN)
        assert len(set(lengths.reshape(-1).tolist())) > 1             # the scale does differ between parents
        if [[(c[1], c[3]) for c in row] for row in want64] != [[(c[1], c[3]) for c in row] for row in plain]:
            reordered.append((V, W))
    print(f"  crafted steps whose chosen list differs from the all-ones table's: {reordered}")
    assert reordered


@pytest.mark.parametrize("V,W", F.CRAFTED_SHAPES)
def test_crafted_steps_meet_their_margin(V, W):
    inputs, lengths, scale, want64, want32, plain, total, seed, gap, edge = F.crafted_case(V, W, MARGIN)
    print(f"  V={V} W={W} seed {seed}: key gap {gap:.3e} top-K boundary gap {edge:.3e}")
    assert gap >= MARGIN and edge >= MARGIN
    assert [[(c[1], c[3]) for c in row] for row in want32] == [[(c[1], c[3]) for c in row] for row in want64]
    done = inputs[6]
    assert bool((lengths[~done] == F.CRAFTED_STEP).all()) and bool(((lengths[done] >= 1) & (lengths[done] <= 2)).all())


@pytest.mark.parametrize("W", sorted(F.EARLY))
def test_early_exit_cases_finish_early_or_never_and_meet_their_margin(W):
    T = F.EARLY_SPEC["T"]
    assert (T, F.EARLY_SPEC["B"], F.EARLY_SPEC["V"]) == (8, 5, 37)
    tokens, lengths, sums, s_star, gap, edge = F.restated_early(W, False)
    print(f"  W={W}: s* {s_star}, key gap {gap:.3e}")
    assert s_star is not None and s_star < T - 2 and gap >= MARGIN and edge >= MARGIN
    assert int(lengths.max()) > 0                                     # not everything ends at step 0
    low = F.restated_early(W, False, torch.float32)
    assert np.array_equal(low[0], tokens) and low[3] == s_star
    tokens, lengths, sums, never, gap, edge = F.restated_early(W, True)
    print(f"  W={W}, sample {F.EARLY_SAMPLE} without END: s* {never}, key gap {gap:.3e}")
    assert never is None and gap >= MARGIN and edge >= MARGIN
    assert int(lengths[F.EARLY_SAMPLE].max()) == T and int(np.delete(lengths, F.EARLY_SAMPLE, 0).max()) < T - 2
    low = F.restated_early(W, True, torch.float32)
    assert np.array_equal(low[0], tokens) and low[3] is None


# ---------------------------------------------------------------------------------------------------------------------
# the CPU route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triple", F.TRIPLES_CPU, ids=triple_id)
def test_cpu_route_reproduces_the_restatement(triple):
    name, W, alpha = triple
    spec, module, inputs = module_of(F.case(*triple), dropout_rate=0.3)      # dropout inactive in eval()
    tokens, lengths, logprobs = module.beam_decode(**inputs, max_seq_len=spec["T"], beam_width=W, length_penalty=alpha,
                                                   **COMMON)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and logprobs.dtype == torch.float32
    assert tokens.shape == (spec["B"], W, spec["T"]) and lengths.shape == (spec["B"], W) == logprobs.shape
    want, want32 = F.restated_case(*triple), F.restated_case(*triple, torch.float32)
    assert np.array_equal(tokens.numpy(), want[0]) and np.array_equal(lengths.numpy(), want[1])     # exact
    assert np.isfinite(want[2]).all()
    scale = max(1.0, float(np.abs(want[2]).max()))
    got = logprobs.double().numpy()
    print(f"  {triple_id(triple)}: |got - fp32 restatement| = {float(np.abs(got - want32[2]).max()):.3e} "
          f"|got - f64| = {float(np.abs(got - want[2]).max()):.3e} scale {scale:.3e}")
    assert attributed_ok(logprobs, torch.from_numpy(want32[2]), torch.from_numpy(want[2]), TOL, scale)
    assert ((tokens >= 0).sum(-1) == lengths).all()
    for n in (1, 2, spec["T"]):                                       # the exit changes no bit
        assert same(module.beam_decode(**inputs, max_seq_len=spec["T"], beam_width=W, length_penalty=alpha, early_exit=n,
                                       **COMMON), (tokens, lengths, logprobs))


@pytest.mark.parametrize("name,W", [("greedy_b1_v37_t1", 1), ("greedy_b5_v37_t4", 3), ("greedy_b5_v1000_t8", 8),
                                    ("greedy_b5_v1000_t8", 12)])
def test_no_penalty_with_an_early_exit_is_the_default_call_bit_for_bit(name, W):
    spec, module, inputs = module_of(beam_cases.case(name, W))
    args = dict(inputs, max_seq_len=spec["T"], beam_width=W, **COMMON)
    default = module.beam_decode(**args)
    for n in (1, 2, spec["T"]):
        assert same(module.beam_decode(**args, length_penalty=0.0, early_exit=n), default), n
    assert same(module.beam_decode(**args, length_penalty=0.0, early_exit=0), default)
    assert same(module.beam_decode(**args, length_penalty=0, early_exit=1), default)


@pytest.mark.parametrize("W", sorted(F.EARLY))
def test_cpu_loops_leave_right_after_the_last_hypothesis_finished(W):
    spec, module, inputs = module_of(F.early_case(W, False))
    T, s_star = spec["T"], F.restated_early(W, False)[3]
    args = dict(inputs, max_seq_len=T, beam_width=W, **COMMON)
    default = module.beam_decode(**args)
    want = F.restated_early(W, False)
    assert np.array_equal(default[0].numpy(), want[0]) and np.array_equal(default[1].numpy(), want[1])
    for n in (1, 2, T):
        with mock.patch.object(module, "_compute_logprobs", wraps=module._compute_logprobs) as spy:
            got = module.beam_decode(**args, early_exit=n)
        assert spy.call_count == s_star + 1 and same(got, default), (n, spy.call_count)
        with mock.patch.object(module, "_compute_logprobs", wraps=module._compute_logprobs) as spy:
            keyed = module.beam_decode(**args, early_exit=n, length_penalty=1.0)
        assert spy.call_count <= T and same(keyed, module.beam_decode(**args, length_penalty=1.0))
    with mock.patch.object(module, "_compute_logprobs", wraps=module._compute_logprobs) as spy:
        module.beam_decode(**args)
    assert spy.call_count == T                                        # the default call pays for every step
    if W == 1:
        greedy_args = dict(inputs, max_seq_len=T, **COMMON)
        full = module.greedy_decode(**greedy_args)
        assert same(full, (default[0][:, 0], default[1][:, 0], default[2][:, 0]))
        for n in (1, 2, T):
            with mock.patch.object(module, "_compute_logprobs", wraps=module._compute_logprobs) as spy:
                got = module.greedy_decode(**greedy_args, early_exit=n)
            assert spy.call_count == s_star + 1 and same(got, full)
    spec, module, inputs = module_of(F.early_case(W, True))           # one sample never ends: every step is run
    args = dict(inputs, max_seq_len=T, beam_width=W, **COMMON)
    with mock.patch.object(module, "_compute_logprobs", wraps=module._compute_logprobs) as spy:
        got = module.beam_decode(**args, early_exit=1)
    assert spy.call_count == T and same(got, module.beam_decode(**args))


def test_argument_errors_come_before_any_work():
    spec, module, inputs = module_of(beam_cases.case("greedy_b5_v37_t4", 2))
    args = dict(inputs, max_seq_len=2, **COMMON)
    with mock.patch.object(module, "_compute_logprobs", side_effect=AssertionError("no work expected")):
        for bad in (-0.5, -1e-9, math.inf, -math.inf, math.nan, "1", None, True):
            with pytest.raises(_lib.PtgnnAmdError, match="length_penalty"):
                module.beam_decode(**args, beam_width=2, length_penalty=bad)
        for bad in (-1, 1.0, 0.5, "2", None, True):
            with pytest.raises(_lib.PtgnnAmdError, match="early_exit"):
                module.beam_decode(**args, beam_width=2, early_exit=bad)
            with pytest.raises(_lib.PtgnnAmdError, match="early_exit"):
                module.greedy_decode(**args, early_exit=bad)
        with pytest.raises(_lib.PtgnnAmdError, match="beam_width"):  # the old checks hold on the new route
            module.beam_decode(**args, beam_width=0, length_penalty=1.0)
        with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
            module.beam_decode(**dict(args, input_element_ids=inputs["input_element_ids"] - 2000), beam_width=2,
                               early_exit=1)
        with pytest.raises(_lib.PtgnnAmdError, match="float32"):     # a table that leaves float32
            module.beam_decode(**dict(args, max_seq_len=300), beam_width=2, length_penalty=120.0)
        tokens, lengths, logprobs = module.beam_decode(**dict(args, max_seq_len=0), beam_width=3, length_penalty=1.0,
                                                       early_exit=1)
    assert tokens.shape == (spec["B"], 3, 0) and logprobs.tolist() == [[0.0, -math.inf, -math.inf]] * spec["B"]
    parameters = inspect.signature(sequence.GruCopyingDecoder.beam_decode).parameters
    assert (parameters["length_penalty"].default, parameters["early_exit"].default) == (0.0, 0)
    assert inspect.signature(sequence.GruCopyingDecoder.greedy_decode).parameters["early_exit"].default == 0


def test_graph2seq_module_forwards_the_new_keywords():
    import graph2seq_cases
    from ptgnn_amd import reduceops
    from ptgnn_amd.gnn import GnnOutput
    parameters = inspect.signature(heads.Graph2SeqModule.beam_decode_finishing).parameters
    assert list(parameters)[1:] == ["encoder_mb_data", "input_element_ids", "start_id", "end_id", "max_seq_len",
                                    "beam_width", "top_k", "length_penalty", "early_exit"]
    assert (parameters["top_k"].default, parameters["length_penalty"].default, parameters["early_exit"].default) \
        == (100, 0.0, 0)
    greedy = inspect.signature(heads.Graph2SeqModule.greedy_decode).parameters
    assert list(greedy)[-1] == "early_exit" and greedy["early_exit"].default == 0
    for p in (parameters, greedy):
        assert all(q.kind == q.KEYWORD_ONLY for name, q in p.items() if name != "self")
    name, spec = graph2seq_cases.CASES[0]
    ns = types.SimpleNamespace(Graph2SeqModule=heads.Graph2SeqModule, GruCopyingDecoder=sequence.GruCopyingDecoder,
                               MultiheadSelfAttentionVarSizedElementReduce=reduceops.MultiheadSelfAttentionVarSizedElementReduce,
                               SimpleVarSizedElementReduce=reduceops.SimpleVarSizedElementReduce)
    torch.manual_seed(spec["seed"])
    module = graph2seq_cases.build(spec, ns, GnnOutput).eval()
    seen = {}

    def decoder_call(which):
        def call(**kwargs):
            seen[which] = kwargs
            return which
        return call
    encoder = graph2seq_cases.call_args(spec, graph2seq_cases.make_inputs(spec, torch.Generator().manual_seed(77)),
                                        to=lambda t: t)["encoder_mb_data"]
    ids = torch.zeros(encoder["backbone_nodes"].shape[0], dtype=torch.int64)
    common = dict(encoder_mb_data=encoder, input_element_ids=ids, start_id=START_ID, end_id=END_ID, max_seq_len=5)
    with mock.patch.object(module._decoder, "beam_decode", decoder_call("beam")), \
            mock.patch.object(module._decoder, "greedy_decode", decoder_call("greedy")):
        assert module.beam_decode_finishing(**common, beam_width=3, length_penalty=0.6, early_exit=2) == "beam"
        assert module.greedy_decode(**common, early_exit=3) == "greedy"
        assert (seen["beam"]["length_penalty"], seen["beam"]["early_exit"], seen["beam"]["beam_width"]) == (0.6, 2, 3)
        assert seen["greedy"]["early_exit"] == 3 and seen["greedy"]["top_k"] == 100
        module.beam_decode(**common, beam_width=3)                    # the pinned call passes neither keyword
        assert "length_penalty" not in seen["beam"] and "early_exit" not in seen["beam"]
        module.greedy_decode(**common)
        assert seen["greedy"]["early_exit"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_(?:search|greedy)_[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "_search_" in s or "_greedy_" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    assert lib.ptgnn_amd_version() == 102 == _lib.MIN_VERSION        # additive: the version stays
    old = re.search(r"\bptgnn_amd_beam_step_f32\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(old.split(",")) == 31 == len(_lib.SIGNATURES["ptgnn_amd_beam_step_f32"][1])     # the old signatures stay
    old = re.search(r"\bptgnn_amd_decode_step_f32\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(old.split(",")) == 25 == len(_lib.SIGNATURES["ptgnn_amd_decode_step_f32"][1])
    assert "DEPENDENT" in header and "key_scale" in header


def test_finish_counters_have_their_own_range_and_keyword(lib):
    names = ["beam_step_links", "beam_backtrack"]
    keywords = ("aggregation", "char_cnn", "heads", "sequence", "decode", "beam", "half", "edge16", "half_training",
                "edge16_dst")
    everything_else = ops.launch_counts(**{k: True for k in keywords})
    for kw in [{}] + [{k: True} for k in keywords]:
        assert not set(names) & set(ops.launch_counts(**kw)), kw
    assert not set(names) & set(everything_else)
    assert list(ops.launch_counts(beam=True)) == list(ops.launch_counts()) + ["beam_step"]     # unchanged
    assert list(ops.launch_counts(beam_finish=True)) == list(ops.launch_counts()) + names
    assert list(ops.launch_counts(beam_finish=True, **{k: True for k in keywords})) == list(everything_else) + names
    first = 704
    assert [lib.ptgnn_amd_launch_name(first + i) for i in range(3)] == [n.encode() for n in names] + [None]
    assert lib.ptgnn_amd_launch_name(first - 1) is None
    assert lib.ptgnn_amd_launch_count(first + 1) == ops.launch_counts(beam_finish=True)["beam_backtrack"]
    assert lib.ptgnn_amd_launch_count(first + 2) == -1 and lib.ptgnn_amd_launch_count(first - 1) == -1
    before = {k: v - 1 for k, v in ops.launch_counts(beam_finish=True).items()}
    assert set(names) <= set(ops.launches_since(before))              # launches_since sees the range
    for start, count in ((0, 13), (64, 17), (128, 4), (192, 4), (256, 3), (320, 1), (384, 1), (448, 2), (512, 2), (576, 3),
                         (640, 1)):                                   # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(start + count) is None and lib.ptgnn_amd_launch_name(start + count - 1) is not None


def test_argument_checks_without_a_gpu(lib):
    size = lib.ptgnn_amd_beam_step_workspace_bytes
    fake = ctypes.c_void_p(4096)                                      # never dereferenced: every call fails its checks first

    def links_step(scores=fake, ld=37, B=5, I=9, vocab=37, top_k=37, W=2, unk=1, end=3, step=0, steps=4, table=fake,
                   done=fake, out=fake, links=fake, live=fake, ws=fake, short=0):
        ws_bytes = size(B, I, vocab, top_k, W)
        return lib.ptgnn_amd_search_step_links_f32(scores, ld, fake, fake, fake, fake, fake, fake, B, I, vocab, top_k, W, unk,
                                                   end, step, steps, table, fake, done, fake, out, fake, fake, fake, fake,
                                                   links, live, None, ws, max(ws_bytes - short, 0), None)

    for bad in (dict(vocab=0, ld=0), dict(vocab=-3), dict(top_k=0), dict(top_k=-1), dict(B=-1), dict(I=-1), dict(ld=36),
                dict(W=0), dict(W=-1), dict(W=9), dict(W=4, top_k=3), dict(W=4, vocab=3, ld=3, unk=1, end=2),
                dict(step=4), dict(step=-1), dict(steps=0), dict(unk=37), dict(unk=-1), dict(end=-1), dict(end=37),
                dict(scores=None), dict(done=None), dict(out=None), dict(ws=None), dict(short=1), dict(table=None),
                dict(links=None)):
        assert links_step(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"beam_step"), bad
    assert links_step(vocab=2 ** 31 - 1, ld=2 ** 31 - 1, top_k=100) == -2
    assert lib.ptgnn_amd_last_error().startswith(b"beam_step")
    assert links_step(B=2 ** 31) == -2 and links_step(I=2 ** 31) == -2
    assert links_step(B=2 ** 27, W=8, steps=4) == -2                        # B W T beyond int32
    assert links_step(B=2 ** 24, W=8, steps=8) == -2                        # 2 B W T, the pairs, beyond int32
    assert links_step(B=0, scores=None, done=None, out=None, ws=None, table=None, links=None) == 0   # nothing to do: no launch

    def back(links=fake, B=5, W=2, run=3, steps=4, tokens=fake):
        return lib.ptgnn_amd_search_backtrack(links, B, W, run, steps, tokens, None)

    for bad in (dict(B=-1), dict(W=0), dict(W=9), dict(steps=0), dict(run=-1), dict(run=5), dict(links=None),
                dict(tokens=None)):
        assert back(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"beam_backtrack:"), bad
    assert back(B=2 ** 31) == -2 and back(B=2 ** 24, W=8, steps=8) == -2
    assert lib.ptgnn_amd_last_error().startswith(b"beam_backtrack:")
    assert back(B=0, links=None, tokens=None) == 0 and back(B=0, run=0, links=None, tokens=None) == 0

    def greedy(scores=fake, ld=37, B=5, I=9, vocab=37, top_k=37, unk=1, end=3, step=0, steps=4, done=fake, live=fake):
        return lib.ptgnn_amd_greedy_step_live_f32(scores, ld, fake, fake, fake, fake, fake, fake, B, I, vocab, top_k, unk, end,
                                                  step, steps, done, fake, fake, fake, fake, live, None, fake, 0, None)

    for bad in (dict(vocab=0, ld=0), dict(top_k=0), dict(B=-1), dict(I=-1), dict(ld=36), dict(step=4), dict(step=-1),
                dict(steps=0), dict(unk=37), dict(end=-1), dict(scores=None), dict(done=None), dict(live=None)):
        assert greedy(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"decode_step:"), bad
    assert greedy(B=2 ** 31) == -2
    assert greedy(B=0, scores=None, done=None, live=None) == 0
    with pytest.raises(_lib.PtgnnAmdError, match="GPU"):              # the wrappers have no CPU path
        ops.beam_step_links(torch.zeros(4, 5), None, torch.zeros(0, 2), torch.zeros(2, 2), (None, torch.zeros(0), None), 3,
                            1, 3, 0, torch.ones(3), tuple(torch.zeros(2, 2) for _ in range(3)),
                            tuple(torch.zeros(2, 2) for _ in range(3)), torch.zeros(4), torch.zeros(4),
                            torch.zeros(2, 2, 2, 2, dtype=torch.int32))
    with pytest.raises(_lib.PtgnnAmdError, match="GPU"):
        ops.beam_backtrack(torch.zeros(2, 2, 2, 2, dtype=torch.int32), 1, torch.zeros(2, 2, 2, dtype=torch.int64))
