"""GruCopyingDecoder.beam_decode without a GPU: the input condition of every (case, width) pair the CPU and GPU tests use
(every decision at least MARGIN from flipping in float64), the CPU route against the float64 / float32 restatement of
tests/beam_cases.py, width 1 against greedy_decode, ordering and bookkeeping (descending scores, a finished hypothesis
keeps its score, every returned sequence re-scored under teacher forcing), and the C ABI of csrc/beam_step.hip as far as it
goes without a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from agg_paths import TOL, attributed_ok
from beam_cases import SEEDED, WIDTHS_CPU, WIDTHS_GPU, case, restated_case
from decoder_cases import UNK_ID, build
from greedy_cases import CASES, END_ID, MARGIN, START_ID, TOP_K, inputs_of, load, state_of
from ptgnn_amd import _lib, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [name for name, _ in CASES]
PAIRS = [(name, W) for name, _ in CASES for W in sorted(set(WIDTHS_CPU) | set(WIDTHS_GPU))]
SYMBOLS = sorted(["ptgnn_amd_beam_step_workspace_bytes", "ptgnn_amd_beam_step_f32"])
COMMON = dict(start_id=START_ID, end_id=END_ID, top_k=TOP_K)


def module_of(name, W, dropout_rate=0.0):
    spec, state, inputs = case(name, W)
    module = build(spec, sequence, dropout_rate).eval()
    module.load_state_dict(state, strict=True)
    return spec, module, inputs


def scores_ok(got, name, W, what):
    """The bar tests/test_greedy_cpu.py holds `logprobs` to, with the float32 restatement as the fp32 reference."""
    exact, want32 = restated_case(name, W)[2], restated_case(name, W, torch.float32)[2]
    scale = max(1.0, float(np.abs(exact).max()))
    got = np.asarray(got, dtype=np.float64)
    print(f"    {what}: |got - fp32 restatement| = {float(np.abs(got - want32).max()):.3e} "
          f"|got - f64| = {float(np.abs(got - exact).max()):.3e} scale {scale:.3e}")
    return attributed_ok(torch.as_tensor(got), torch.from_numpy(want32), torch.from_numpy(exact), TOL, scale)


@pytest.mark.parametrize("name,W", PAIRS, ids=[f"{n}-w{w}" for n, w in PAIRS])
def test_every_decision_of_a_case_is_a_margin_away_from_flipping(name, W):
    spec, state, inputs = case(name, W)
    if (name, W) not in SEEDED:                                       # the fixture itself
        fx = load(name)
        assert all(torch.equal(inputs[k], inputs_of(fx)[k]) for k in inputs)
    tokens, lengths, scores, gap, edge = restated_case(name, W)
    print(f"  {name} W={W} (seed {SEEDED.get((name, W))}): decision gap {gap:.3e}, top-K boundary gap {edge:.3e}")
    assert gap >= MARGIN and edge >= MARGIN                           # no sample is left out of either minimum
    assert tokens.shape == (spec["B"], W, spec["T"]) and np.isfinite(scores).all()
    low = restated_case(name, W, torch.float32)                       # fp32 takes the same decisions
    assert np.array_equal(low[0], tokens) and np.array_equal(low[1], lengths)


def test_the_cases_cover_end_copies_vocabulary_entries_keys_and_reordered_parents():
    seen = set()
    for name, spec in CASES:
        tokens, lengths, scores, _, _ = restated_case(name, 3)
        ids = set(case(name, 3)[2]["input_element_ids"].tolist())
        seen |= {"end"} if (lengths < spec["T"]).any() else set()
        seen |= {"full"} if (lengths == spec["T"]).any() else set()
        seen |= {"outside"} if (tokens >= spec["V"]).any() else set()
        seen |= {"vocabulary"} if any(t not in ids for t in tokens[tokens >= 0].tolist()) else set()
        seen |= {"copy"} if any(t in ids for t in tokens[tokens >= 0].tolist()) else set()
        if spec["T"] > 1 and (tokens[:, 1:, 0] != tokens[:, :1, 0]).any():
            seen |= {"branches"}                                      # slots of a sample that differ in their first token
    assert seen == {"end", "full", "outside", "vocabulary", "copy", "branches"}


@pytest.mark.parametrize("W", WIDTHS_CPU)
@pytest.mark.parametrize("name", IDS)
def test_cpu_route_reproduces_the_restatement(name, W):
    spec, module, inputs = module_of(name, W, dropout_rate=0.3)      # dropout inactive in eval()
    tokens, lengths, logprobs = module.beam_decode(**inputs, max_seq_len=spec["T"], beam_width=W, **COMMON)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and logprobs.dtype == torch.float32
    assert tokens.shape == (spec["B"], W, spec["T"]) and lengths.shape == (spec["B"], W) == logprobs.shape
    want = restated_case(name, W)
    assert np.array_equal(tokens.numpy(), want[0]) and np.array_equal(lengths.numpy(), want[1])
    assert scores_ok(logprobs.numpy(), name, W, f"{name} W={W}")
    assert bool((logprobs[:, :-1] >= logprobs[:, 1:]).all())         # descending per sample, slot 0 the best
    assert ((tokens >= 0).sum(-1) == lengths).all()


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_width_one_is_greedy_decoding(name, spec):
    fx = load(name)
    module = build(spec, sequence).eval()
    module.load_state_dict(state_of(fx), strict=True)
    args = dict(inputs_of(fx), start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"], top_k=TOP_K)
    tokens, lengths, logprobs = module.beam_decode(**args, beam_width=1)
    want = module.greedy_decode(**args)
    assert torch.equal(tokens[:, 0], want[0]) and torch.equal(lengths[:, 0], want[1])
    assert np.array_equal(tokens[:, 0].numpy(), fx["token_ids"])
    assert torch.equal(logprobs[:, 0], want[2])
    half = module.beam_decode(**dict(args, input_memories=args["input_memories"].bfloat16().float()), beam_width=2)
    half16 = module.beam_decode(**dict(args, input_memories=args["input_memories"].bfloat16()), beam_width=2)
    for a, b in zip(half, half16):                                   # bf16 memories are up-cast on entry
        assert torch.equal(a, b)


def test_a_finished_hypothesis_keeps_its_score_to_the_end():
    name, W = "greedy_b5_v1000_t8", 3
    spec, module, inputs = module_of(name, W)
    runs = [module.beam_decode(**inputs, max_seq_len=T, beam_width=W, **COMMON) for T in range(1, spec["T"] + 1)]
    kept = 0
    for T, (earlier, later) in enumerate(zip(runs, runs[1:]), start=1):
        for b in range(spec["B"]):
            after = {tuple(later[0][b, p, :int(later[1][b, p])].tolist()): later[2][b, p] for p in range(W)
                     if int(later[1][b, p]) <= T}
            for p in range(W):
                if int(earlier[1][b, p]) < T:                        # finished within the first T steps
                    key = tuple(earlier[0][b, p, :int(earlier[1][b, p])].tolist())
                    if key in after:                                  # still in the beam: the same bits
                        assert torch.equal(after[key], earlier[2][b, p])
                        kept += 1
    assert kept > 0


# a returned score is the sum of at most T + 1 = 9 fp32 log-probabilities of magnitude below 32 (one ulp: 3.8e-6), each
# computed twice on different routes (one GRU step at a time in the loop, the whole sequence at once here): three ulps a
# term, 9 * 3 * 3.8e-6
RESCORE_TOL = 1e-4


@pytest.mark.parametrize("name,W", [("greedy_b5_v37_t4", 3), ("greedy_b5_v1000_t8", 3), ("greedy_b1_v1000_t4", 8)])
def test_histories_are_consistent_with_their_scores_under_teacher_forcing(name, W):
    spec, module, inputs = module_of(name, W)
    V, T, B = spec["V"], spec["T"], spec["B"]
    tokens, lengths, logprobs = module.beam_decode(**inputs, max_seq_len=T, beam_width=W, **COMMON)
    index, ids = inputs["input_memories_origin_idx"], inputs["input_element_ids"]
    for p in range(W):
        chosen = torch.full((B, T + 1), END_ID, dtype=torch.int64)    # what each step chose: the tokens, then END
        for b in range(B):
            chosen[b, :int(lengths[b, p])] = tokens[b, p, :int(lengths[b, p])]
        fed = torch.cat((torch.full((B, 1), START_ID), torch.where(chosen < V, chosen, UNK_ID)[:, :T - 1]), dim=1)
        with torch.no_grad():
            copy, target, _ = module._compute_logprobs(inputs["initial_states"], inputs["input_memories"], index, fed)
        for b in range(B):
            steps = min(int(lengths[b, p]) + 1, T)                    # END's step too, where there was one
            total = 0.0
            for step in range(steps):
                e = int(chosen[b, step])
                row = target[b, step]
                entry = -math.inf
                if e < V and e in torch.sort(row, descending=True, stable=True).indices[:TOP_K].tolist():
                    entry = float(row[e])
                group = copy[(index == b) & (ids == e), step]
                if group.numel():
                    entry = float(np.logaddexp(entry, float(torch.logsumexp(group.double(), 0))))
                total += entry
            assert abs(total - float(logprobs[b, p])) <= RESCORE_TOL, (b, p, total, float(logprobs[b, p]))


def test_cpu_route_edge_cases_and_argument_errors():
    name, spec = CASES[1]
    fx = load(name)
    module = build(spec, sequence, dropout_rate=0.2).eval()
    module.load_state_dict(state_of(fx), strict=True)
    inp = inputs_of(fx)
    common = dict(start_id=START_ID, end_id=END_ID)
    tokens, lengths, logprobs = module.beam_decode(**inp, max_seq_len=0, beam_width=3, **common)
    assert tokens.shape == (spec["B"], 3, 0) and lengths.tolist() == [[0] * 3] * spec["B"]
    assert logprobs.tolist() == [[0.0, -math.inf, -math.inf]] * spec["B"]        # the slots before step 0
    none = dict(inp, initial_states=inp["initial_states"][:0], input_memories=inp["input_memories"][:0],
                input_memories_origin_idx=inp["input_memories_origin_idx"][:0], input_element_ids=inp["input_element_ids"][:0])
    tokens, lengths, logprobs = module.beam_decode(**none, max_seq_len=3, beam_width=2, **common)
    assert tokens.shape == (0, 2, 3) and lengths.shape == (0, 2) and logprobs.shape == (0, 2)
    with pytest.raises(_lib.PtgnnAmdError, match="beam_width"):
        module.beam_decode(**inp, max_seq_len=2, beam_width=0, **common)
    with pytest.raises(_lib.PtgnnAmdError, match="beam_width"):      # above the vocabulary: 37
        module.beam_decode(**inp, max_seq_len=2, beam_width=38, **common)
    with pytest.raises(_lib.PtgnnAmdError, match="beam_width"):      # above top_k
        module.beam_decode(**inp, max_seq_len=2, beam_width=5, top_k=4, **common)
    module.beam_decode(**inp, max_seq_len=1, beam_width=37, **common)  # the CPU route takes any width up to min(top_k, V)
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        module.beam_decode(**dict(inp, input_element_ids=inp["input_element_ids"] - 2000), max_seq_len=2, beam_width=2,
                           **common)
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        module.beam_decode(**dict(inp, input_element_ids=inp["input_element_ids"][:-1]), max_seq_len=2, beam_width=2,
                           **common)
    with pytest.raises(_lib.PtgnnAmdError, match="start_id"):
        module.beam_decode(**inp, max_seq_len=2, beam_width=2, start_id=START_ID, end_id=37)
    with pytest.raises(_lib.PtgnnAmdError, match="dropout"):
        module.train().beam_decode(**inp, max_seq_len=2, beam_width=2, **common)


def test_graph2seq_module_forwards_beam_decode():
    import inspect
    from ptgnn_amd import heads
    parameters = inspect.signature(heads.Graph2SeqModule.beam_decode).parameters
    assert list(parameters)[1:] == ["encoder_mb_data", "input_element_ids", "start_id", "end_id", "max_seq_len",
                                    "beam_width", "top_k"]
    assert parameters["top_k"].default == 100
    assert all(p.kind == p.KEYWORD_ONLY for name, p in parameters.items() if name != "self")


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    from ptgnn_amd import build as B
    assert "beam_step.hip" in B.SOURCES
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_beam_step[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "beam" in s) == declared
    assert not [s for s in SYMBOLS if "decode_step" in s]
    assert lib.ptgnn_amd_version() == 102


def test_beam_counter_has_its_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    everything_else = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True)
    for kw in ({}, dict(aggregation=True), dict(char_cnn=True), dict(heads=True), dict(sequence=True), dict(decode=True)):
        assert "beam_step" not in ops.launch_counts(**kw), kw
    assert "beam_step" not in everything_else
    assert list(ops.launch_counts(beam=True)) == list(ops.launch_counts()) + ["beam_step"]
    assert list(ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True, beam=True)) \
        == list(everything_else) + ["beam_step"]
    first = 384
    assert lib.ptgnn_amd_launch_name(first) == b"beam_step"
    assert lib.ptgnn_amd_launch_name(first + 1) is None and lib.ptgnn_amd_launch_name(first - 1) is None
    assert lib.ptgnn_amd_launch_count(first) == ops.launch_counts(beam=True)["beam_step"]
    assert lib.ptgnn_amd_launch_count(first + 1) == -1 and lib.ptgnn_amd_launch_count(first - 1) == -1
    before = {k: v - 1 for k, v in ops.launch_counts(beam=True).items()}
    assert "beam_step" in ops.launches_since(before)                   # launches_since sees the range
    for end in (13, 64 + 17, 128 + 4, 192 + 4, 256 + 3, 320 + 1):    # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(end) is None and lib.ptgnn_amd_launch_name(end - 1) is not None


def test_workspace_and_argument_checks_without_a_gpu(lib):
    from ptgnn_amd import ops
    size = lib.ptgnn_amd_beam_step_workspace_bytes
    # (samples, memories, vocab, top_k, beam width): nothing to measure for what the entry refuses
    for sizes in ((0, 9, 37, 37, 2), (5, 9, 0, 1, 1), (5, 9, 37, 0, 1), (5, -1, 37, 37, 2), (-2, 9, 37, 37, 2),
                  (5, 9, 37, 37, 0), (5, 9, 37, 37, 9), (5, 9, 37, 3, 4), (5, 9, 3, 37, 4), (2 ** 31, 9, 37, 37, 2)):
        assert size(*sizes) == 0, sizes
    assert size(5, 9, 37, 37, 2) >= 4 * 9 * 2 + 16 * 5 * 2 * 2       # a float per (memory, slot), 16 bytes a candidate
    fake = ctypes.c_void_p(4096)                                      # never dereferenced: every call fails its checks first

    def call(scores=fake, ld=37, B=5, I=9, vocab=37, top_k=37, W=2, unk=1, end=3, step=0, steps=4, done=fake, out=fake,
             ws=fake, short=0):
        ws_bytes = size(B, I, vocab, top_k, W)
        return lib.ptgnn_amd_beam_step_f32(scores, ld, fake, fake, fake, fake, fake, fake, B, I, vocab, top_k, W, unk, end,
                                           step, steps, fake, done, fake, fake, out, fake, fake, fake, fake, fake, None,
                                           ws, max(ws_bytes - short, 0), None)

    for bad in (dict(vocab=0, ld=0), dict(vocab=-3), dict(top_k=0), dict(top_k=-1), dict(B=-1), dict(I=-1), dict(ld=36),
                dict(W=0), dict(W=-1), dict(W=9), dict(W=4, top_k=3), dict(W=4, vocab=3, ld=3, unk=1, end=2),
                dict(step=4), dict(step=-1), dict(steps=0), dict(unk=37), dict(unk=-1), dict(end=-1), dict(end=37),
                dict(scores=None), dict(done=None), dict(out=None), dict(ws=None), dict(short=1)):
        assert call(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"beam_step:"), bad
    assert call(vocab=2 ** 31 - 1, ld=2 ** 31 - 1, top_k=100) == -2 and lib.ptgnn_amd_last_error().startswith(b"beam_step:")
    assert call(B=2 ** 31) == -2 and call(I=2 ** 31) == -2
    assert call(B=2 ** 27, W=8, steps=4) == -2                        # B W T beyond int32
    assert call(B=0, scores=None, done=None, out=None, ws=None) == 0  # nothing to do: no launch
    with pytest.raises(_lib.PtgnnAmdError, match="GPU"):              # the wrapper has no CPU path
        ops.beam_step(torch.zeros(4, 5), None, torch.zeros(0, 2), torch.zeros(2, 2), (None, torch.zeros(0), None), 3, 1, 3,
                      0, tuple(torch.zeros(2, 2) for _ in range(4)), tuple(torch.zeros(2, 2) for _ in range(4)),
                      torch.zeros(4), torch.zeros(4))
