"""GruCopyingDecoder.greedy_decode without a GPU: the fixtures' input condition (every decision at least MARGIN from
flipping in float64), the restatement of the reference's dict algorithm and the CPU route of the method against the
reference's fixtures, and the C ABI of csrc/decode_step.hip as far as it goes without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from agg_paths import TOL, attributed_ok
from decoder_cases import build
from greedy_cases import (CASES, END_ID, MARGIN, START_ID, TOP_K, inputs_of, load, make_inputs, restated_decode, state_of,
                          weights_from)
from ptgnn_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [name for name, _ in CASES]
SYMBOLS = sorted(["ptgnn_amd_decode_step_workspace_bytes", "ptgnn_amd_decode_step_f32"])


def logprobs_ok(got, fx, exact, what):
    """The attributed bar on the summed log-probabilities: the reference's fp32 result, the float64 restatement."""
    scale = max(1.0, float(np.abs(exact).max()))
    print(f"    {what}: |got - reference| = {float(np.abs(np.asarray(got, dtype=np.float64) - fx['logprobs']).max()):.3e} "
          f"|got - f64| = {float(np.abs(np.asarray(got, dtype=np.float64) - exact).max()):.3e} scale {scale:.3e}")
    return attributed_ok(torch.as_tensor(got), torch.from_numpy(fx["logprobs"]), torch.from_numpy(exact), TOL, scale)


@pytest.fixture(scope="module")
def restated():
    """name -> {dtype: restated_decode(...)}: computed once, shared, left unchanged."""
    out = {}
    for name, spec in CASES:
        fx = load(name)
        out[name] = {dt: restated_decode(weights_from(fx, dt), inputs_of(fx), spec) for dt in (torch.float64, torch.float32)}
    return out


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_every_decision_of_a_fixture_is_a_margin_away_from_flipping(name, spec, restated):
    fx = load(name)
    inputs = make_inputs(spec, torch.Generator().manual_seed(9500 + spec["seed"]))
    for k, v in inputs.items():                                       # the fixture holds the inputs of its case
        assert torch.equal(torch.from_numpy(fx[k]), v), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1 << 20
    _, _, _, gap, edge = restated[name][torch.float64]
    print(f"  {name}: best-vs-second gap {gap:.3e}, top-K boundary gap {edge:.3e}")
    assert gap >= MARGIN and edge >= MARGIN
    ids = inputs["input_element_ids"]
    assert bool((ids >= spec["V"]).any()) and bool((ids < spec["V"]).any())     # both halves of the extended id space


def test_the_fixtures_cover_end_copies_vocabulary_entries_and_keys_outside_the_vocabulary():
    seen = set()
    for name, spec in CASES:
        fx = load(name)
        tokens, ids = fx["token_ids"], set(fx["input_element_ids"].tolist())
        seen |= {"end"} if (fx["lengths"] < spec["T"]).any() else set()
        seen |= {"full"} if (fx["lengths"] == spec["T"]).any() else set()
        seen |= {"outside"} if (tokens >= spec["V"]).any() else set()
        seen |= {"vocabulary"} if any(t not in ids for t in tokens[tokens >= 0].tolist()) else set()
        seen |= {"copy"} if any(t in ids for t in tokens[tokens >= 0].tolist()) else set()
        assert ((tokens >= 0).sum(1) == fx["lengths"]).all() and (tokens[:, 0] >= 0).sum() == (fx["lengths"] > 0).sum()
    assert seen == {"end", "full", "outside", "vocabulary", "copy"}


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_restatement_reproduces_the_reference(name, spec, restated):
    fx = load(name)
    exact = restated[name][torch.float64]
    for dt, (tokens, lengths, logprobs, _, _) in restated[name].items():
        assert np.array_equal(tokens, fx["token_ids"]) and np.array_equal(lengths, fx["lengths"]), dt
        assert logprobs_ok(logprobs, fx, exact[2], f"{name} {dt}")


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_reproduces_the_reference(name, spec, restated):
    fx = load(name)
    module = build(spec, sequence, dropout_rate=0.3).eval()          # dropout inactive in eval()
    module.load_state_dict(state_of(fx), strict=True)
    tokens, lengths, logprobs = module.greedy_decode(**inputs_of(fx), start_id=START_ID, end_id=END_ID,
                                                     max_seq_len=spec["T"], top_k=TOP_K)
    assert tokens.dtype == torch.int64 and lengths.dtype == torch.int64 and logprobs.dtype == torch.float32
    assert np.array_equal(tokens.numpy(), fx["token_ids"]) and np.array_equal(lengths.numpy(), fx["lengths"])
    assert logprobs_ok(logprobs.numpy(), fx, restated[name][torch.float64][2], name)
    half = module.greedy_decode(**dict(inputs_of(fx), input_memories=inputs_of(fx)["input_memories"].bfloat16().float()),
                                start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"])
    half16 = module.greedy_decode(**dict(inputs_of(fx), input_memories=inputs_of(fx)["input_memories"].bfloat16()),
                                  start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"])
    for a, b in zip(half, half16):                                   # bf16 memories are up-cast on entry
        assert torch.equal(a, b)


def test_cpu_route_edge_cases():
    name, spec = CASES[1]
    fx = load(name)
    module = build(spec, sequence).eval()
    module.load_state_dict(state_of(fx), strict=True)
    inp = inputs_of(fx)
    common = dict(start_id=START_ID, end_id=END_ID)
    tokens, lengths, logprobs = module.greedy_decode(**inp, max_seq_len=0, **common)
    assert tokens.shape == (spec["B"], 0) and lengths.tolist() == [0] * spec["B"] and logprobs.tolist() == [0.0] * spec["B"]
    none = dict(inp, initial_states=inp["initial_states"][:0], input_memories=inp["input_memories"][:0],
                input_memories_origin_idx=inp["input_memories_origin_idx"][:0], input_element_ids=inp["input_element_ids"][:0])
    tokens, lengths, logprobs = module.greedy_decode(**none, max_seq_len=3, **common)
    assert tokens.shape == (0, 3) and lengths.shape == (0,) and logprobs.shape == (0,)
    # top_k = 1: only the vocabulary's best entry survives the top K; a copy group of another vocabulary id starts from -inf
    one = module.greedy_decode(**inp, max_seq_len=spec["T"], top_k=1, **common)
    w = weights_from(fx, torch.float64)
    want = restated_decode(w, inp, spec, top_k=1)
    assert want[3] >= MARGIN and want[4] >= MARGIN
    assert np.array_equal(one[0].numpy(), want[0]) and np.array_equal(one[1].numpy(), want[1])
    from ptgnn_amd import _lib
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        module.greedy_decode(**dict(inp, input_element_ids=inp["input_element_ids"] - 2000), max_seq_len=2, **common)
    with pytest.raises(_lib.PtgnnAmdError, match="input_element_ids"):
        module.greedy_decode(**dict(inp, input_element_ids=inp["input_element_ids"][:-1]), max_seq_len=2, **common)
    with pytest.raises(_lib.PtgnnAmdError, match="top_k"):
        module.greedy_decode(**inp, max_seq_len=2, top_k=0, **common)


def test_training_mode_with_dropout_raises():
    from ptgnn_amd import _lib
    name, spec = CASES[0]
    fx = load(name)
    module = build(spec, sequence, dropout_rate=0.2)
    module.load_state_dict(state_of(fx), strict=True)
    args = dict(inputs_of(fx), start_id=START_ID, end_id=END_ID, max_seq_len=spec["T"])
    with pytest.raises(_lib.PtgnnAmdError, match="dropout"):
        module.train().greedy_decode(**args)
    want = module.eval().greedy_decode(**args)
    plain = build(spec, sequence, dropout_rate=0.0).train()          # p = 0: nothing to switch off
    plain.load_state_dict(state_of(fx), strict=True)
    for a, b in zip(want, plain.greedy_decode(**args)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    from ptgnn_amd import _lib, build as B
    assert "decode_step.hip" in B.SOURCES
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_decode_step[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "decode_step" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    pinned = ("vocab_loss", "copy_loss_finish", "segment_scores", "logit_loss", "candidate_scores", "embedding_bag",
              "char_embed", "window_", "graph_norm", "block_attention", "attention_windows")
    assert not [s for s in SYMBOLS if any(p in s for p in pinned)]
    assert "grucopydecoder.py:375-457" in header


def test_decode_counter_has_its_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    everything_else = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True)
    for kw in ({}, dict(aggregation=True), dict(char_cnn=True), dict(heads=True), dict(sequence=True)):
        assert "decode_step" not in ops.launch_counts(**kw), kw
    assert "decode_step" not in everything_else
    assert list(ops.launch_counts(decode=True)) == list(ops.launch_counts()) + ["decode_step"]
    assert list(ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True)) \
        == list(everything_else) + ["decode_step"]
    first = 320
    assert lib.ptgnn_amd_launch_name(first) == b"decode_step" and lib.ptgnn_amd_launch_name(first + 1) is None
    assert lib.ptgnn_amd_launch_name(first - 1) is None
    assert lib.ptgnn_amd_launch_count(first) == ops.launch_counts(decode=True)["decode_step"]
    assert lib.ptgnn_amd_launch_count(first + 1) == -1
    before = {k: v - 1 for k, v in ops.launch_counts(decode=True).items()}
    assert "decode_step" in ops.launches_since(before)                         # launches_since sees the range
    for end in (13, 64 + 17, 128 + 4, 192 + 4, 256 + 3):                     # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(end) is None and lib.ptgnn_amd_launch_name(end - 1) is not None


def test_workspace_and_argument_checks_without_a_gpu(lib):
    # nothing to measure for no samples, no columns or no candidates; the kernel keeps a sample's partials in LDS
    for sizes in ((0, 37, 37), (5, 0, 1), (5, 37, 0), (5, -1, 3), (-2, 37, 37)):
        assert lib.ptgnn_amd_decode_step_workspace_bytes(*sizes) == 0, sizes
    fake = ctypes.c_void_p(4096)                                      # never dereferenced: every call fails its checks first

    def call(scores=fake, ld=37, B=5, I=9, vocab=37, top_k=37, unk=1, end=3, step=0, steps=4, done=fake):
        ws_bytes = lib.ptgnn_amd_decode_step_workspace_bytes(B, vocab, top_k)
        return lib.ptgnn_amd_decode_step_f32(scores, ld, fake, fake, fake, fake, fake, fake, B, I, vocab, top_k, unk, end,
                                             step, steps, done, fake, fake, fake, fake, None, fake, ws_bytes, None)

    for bad in (dict(vocab=0, ld=0), dict(vocab=-3), dict(top_k=0), dict(top_k=-1), dict(B=-1), dict(I=-1), dict(ld=36),
                dict(step=4), dict(step=-1), dict(steps=0), dict(unk=37), dict(end=-1), dict(end=37), dict(scores=None),
                dict(done=None)):
        assert call(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"decode_step:"), bad
    assert call(vocab=2 ** 31 - 1, ld=2 ** 31 - 1, top_k=100) == -2 and lib.ptgnn_amd_last_error().startswith(b"decode_step:")
    assert call(B=2 ** 31) == -2
    assert call(B=0, scores=None, done=None) == 0                     # nothing to do: no launch
    from ptgnn_amd import _lib, ops
    with pytest.raises(_lib.PtgnnAmdError, match="GPU"):              # the wrapper has no CPU path
        ops.decode_step(torch.zeros(2, 5), None, torch.zeros(0), torch.zeros(2), (None, torch.zeros(0), None), 3, 1, 3, 0,
                        *(torch.zeros(2) for _ in range(5)))
