"""Graph2SeqModule (ptgnn_amd.heads) and GruCopyingDecoder.fused_loss without a GPU: the fixtures' input conditions, the
reference's state_dict keys and same-seed initial parameters, the CPU route against the reference fixtures, and the C ABI
of csrc/vocab_loss.hip as far as it goes without a device."""
import ctypes
import os
import re
import types

import pytest
import torch
from torch import nn

import ptgnn_amd
from decoder_cases import CASES as DECODER_CASES
from decoder_cases import build as build_decoder
from decoder_cases import inputs_of as decoder_inputs_of
from decoder_cases import load as load_decoder
from decoder_cases import state_of as decoder_state_of
from graph2seq_cases import CASES, build, call_args, conditions_hold, files, inputs_of, load, make_inputs, state_of
from ptgnn_amd import heads, reduceops, sequence
from ptgnn_amd.gnn import GnnOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_TOL = 2e-5          # the bar of tests/test_decoder_cpu.py, relative to max(1, max |want|)
IDS = [name for name, _ in CASES]
NS = types.SimpleNamespace(Graph2SeqModule=heads.Graph2SeqModule, GruCopyingDecoder=sequence.GruCopyingDecoder,
                           MultiheadSelfAttentionVarSizedElementReduce=reduceops.MultiheadSelfAttentionVarSizedElementReduce,
                           SimpleVarSizedElementReduce=reduceops.SimpleVarSizedElementReduce)
SYMBOLS = sorted(["ptgnn_amd_vocab_loss_workspace_bytes", "ptgnn_amd_vocab_loss_f32",
                  "ptgnn_amd_vocab_loss_backward_workspace_bytes", "ptgnn_amd_vocab_loss_backward_f32",
                  "ptgnn_amd_copy_loss_finish_workspace_bytes", "ptgnn_amd_copy_loss_finish_f32"])
SEQ_COUNTERS = ["vocab_loss", "vocab_loss_backward", "copy_loss_finish"]


def close(got, want, tol=FIXTURE_TOL):
    got, want = torch.as_tensor(got).detach().double(), torch.as_tensor(want).double()
    if got.shape != want.shape:
        return False
    err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"    |got - want| = {err:.3e} (scale {scale:.3e})")
    return err <= tol * scale


def fixture_module(name, spec):
    fx = load(name)
    module = build(spec, NS, GnnOutput)
    module.load_state_dict(state_of(fx), strict=True)
    return fx, module


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_fixture_inputs_meet_the_input_conditions(name, spec):
    fx = load(name)
    inputs = make_inputs(spec, torch.Generator().manual_seed(9000 + spec["seed"]))
    assert conditions_hold(spec, inputs)
    for k, v in inputs.items():                                       # the fixture holds the inputs of its case
        assert torch.equal(torch.from_numpy(fx[k]), v), k
    assert all(os.path.getsize(path) < 700_000 for path in files(name))
    for key in ("loss", "second.loss", "metrics1.loss", "metrics2.loss", "grad.input_states", "grad.output_states"):
        assert key in fx, key


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_state_dict_keys_initial_parameters_and_strict_load(name, spec):
    fx = load(name)
    torch.manual_seed(spec["seed"])
    module = build(spec, NS, GnnOutput)
    want = state_of(fx)
    assert list(module.state_dict()) == list(want)                    # the reference's name-mangled keys, in its order
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k                             # same seed, same draws in the same order
    other = build(spec, NS, GnnOutput)
    other.load_state_dict(want, strict=True)                          # reference -> ptgnn_amd
    assert set(other.state_dict()) == set(want)                       # ptgnn_amd -> reference: the same key set
    assert sorted("grad." + k for k, _ in module.named_parameters()) == sorted(
        k for k in fx if k.startswith("grad.") and not k.endswith("_states"))


def test_reference_attribute_names_and_exports():
    module = build(CASES[0][1], NS, GnnOutput)
    assert isinstance(module._decoder, sequence.GruCopyingDecoder)
    assert module._gnn.output_node_state_dim == CASES[0][1]["D_out"]
    assert isinstance(module._Graph2SeqModule__node_to_graph_representation,
                      reduceops.MultiheadSelfAttentionVarSizedElementReduce)
    keys = list(module.state_dict())
    first_summariser = min(i for i, k in enumerate(keys) if k.startswith("_Graph2SeqModule__node_to_graph_representation."))
    assert all(k.startswith("_decoder.") for k in keys[:first_summariser])
    assert all(k.startswith("_Graph2SeqModule__node_to_graph_representation.") for k in keys[first_summariser:])
    assert isinstance(module, ptgnn_amd.gnn.ModuleWithMetrics)
    assert ptgnn_amd.Graph2SeqModule is heads.Graph2SeqModule
    with pytest.raises(ptgnn_amd.PtgnnAmdError):
        module.forward_sharded()


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_against_the_reference_fixture(name, spec):
    fx, module = fixture_module(name, spec)
    inputs = inputs_of(fx)
    module.reset_metrics()
    states = tuple(inputs[k].clone().requires_grad_(True) for k in ("input_states", "output_states"))
    loss = module(**call_args(spec, inputs, states=states))
    loss.backward()
    assert close(loss, fx["loss"])
    assert close(states[0].grad, fx["grad.input_states"]) and close(states[1].grad, fx["grad.output_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k
    first = module.report_metrics()
    with torch.no_grad():
        assert close(module(**call_args(spec, inputs, second=True)), fx["second.loss"])
    second = module.report_metrics()
    assert list(first) == ["loss"] == list(second)
    assert close(first["loss"], fx["metrics1.loss"]) and close(second["loss"], fx["metrics2.loss"])
    assert float(fx["metrics1.loss"]) != float(fx["metrics2.loss"])
    module.reset_metrics()                                            # a working reset: the first minibatch alone again
    with torch.no_grad():
        module(**call_args(spec, inputs))
    assert close(module.report_metrics()["loss"], fx["metrics1.loss"])


@pytest.mark.parametrize("name,spec", DECODER_CASES, ids=[n for n, _ in DECODER_CASES])
def test_fused_loss_on_cpu_tensors_is_forward_bit_for_bit(name, spec):
    fx = load_decoder(name)
    module = build_decoder(spec, sequence)
    module.load_state_dict(decoder_state_of(fx), strict=True)
    runs, threads = [], torch.get_num_threads()
    torch.set_num_threads(1)            # torch's threaded CPU scatter-adds fold in no fixed order: two runs of `forward`
    try:                                # itself differ in the last bit otherwise
        for fn in (module.forward, module.fused_loss):
            module.zero_grad(set_to_none=True)
            inputs = decoder_inputs_of(fx)
            inputs["input_memories"].requires_grad_(True)
            inputs["initial_states"].requires_grad_(True)
            loss = fn(**inputs)
            loss.backward()
            runs.append([loss.detach()] + [inputs["input_memories"].grad, inputs["initial_states"].grad]
                        + [p.grad.clone() for p in module.parameters()])
    finally:
        torch.set_num_threads(threads)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_cpu_tensors_never_load_the_library(monkeypatch):
    from ptgnn_amd import _lib

    def refuse():
        raise AssertionError("a CPU forward / backward loaded the library")

    monkeypatch.setattr(_lib, "load", refuse)
    name, spec = CASES[0]
    fx, module = fixture_module(name, spec)
    module(**call_args(spec, inputs_of(fx))).backward()
    module.report_metrics()
    dfx = load_decoder(DECODER_CASES[0][0])
    decoder = build_decoder(DECODER_CASES[0][1], sequence)
    decoder.fused_loss(**decoder_inputs_of(dfx)).backward()


def test_a_stand_in_decoder_is_called_through_call():
    class StandIn(nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.tensor(2.0))
            self.seen = None

        def forward(self, **kwargs):
            self.seen = kwargs
            return self.scale * kwargs["input_memories"].sum() + kwargs["initial_states"].sum()

        def fused_loss(self, **kwargs):
            raise AssertionError("fused_loss of a module that is not ptgnn_amd's decoder")

    name, spec = CASES[0]
    fx, module = fixture_module(name, spec)
    stand_in, hooked = StandIn(), []
    stand_in.register_forward_pre_hook(lambda m, args: hooked.append(True))      # hooks run through __call__ only
    module._decoder = stand_in
    inputs = inputs_of(fx)
    loss = module(**call_args(spec, inputs))
    assert hooked == [True]
    assert sorted(stand_in.seen) == sorted(["input_memories", "input_memories_origin_idx", "initial_states",
                                            "target_token_ids", "copyable_elements_idxs",
                                            "copyable_elements_sample_idxs", "target_lengths"])
    assert torch.equal(stand_in.seen["input_memories"], inputs["output_states"][inputs["backbone_nodes"]])
    assert torch.equal(stand_in.seen["input_memories_origin_idx"], inputs["backbone_graphs"])
    assert close(module.report_metrics()["loss"], float(loss.detach()))


def test_the_reference_route_switch_calls_forward_of_the_own_decoder(monkeypatch):
    name, spec = CASES[0]
    fx, module = fixture_module(name, spec)
    assert heads.Graph2SeqModule.use_fused_loss in (True, False)
    calls = []
    monkeypatch.setattr(sequence.GruCopyingDecoder, "fused_loss",
                        lambda self, **kw: calls.append("fused") or self.forward(**kw))
    module.use_fused_loss = True
    module(**call_args(spec, inputs_of(fx)))
    module.use_fused_loss = False
    module(**call_args(spec, inputs_of(fx)))
    assert calls == ["fused"]


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
    assert "vocab_loss.hip" in B.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_(?:vocab_loss|copy_loss_finish)[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "vocab_loss" in s or "copy_loss_finish" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    pinned = ("logit_loss", "candidate_scores", "segment_scores", "embedding_bag", "char_embed", "_window_", "graph_norm",
              "block_attention", "attention_windows")
    assert not [s for s in SYMBOLS if any(p in s for p in pinned)]
    assert "grucopydecoder.py:118-135, 171-212" in open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()


def test_sequence_counters_have_their_own_keyword(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    plain = list(ops.launch_counts())
    assert not set(SEQ_COUNTERS) & set(plain)
    everything_else = ops.launch_counts(aggregation=True, char_cnn=True, heads=True)
    assert not set(SEQ_COUNTERS) & set(everything_else)
    assert list(ops.launch_counts(sequence=True)) == plain + SEQ_COUNTERS
    assert list(ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True)) \
        == list(everything_else) + SEQ_COUNTERS
    before = {k: v - 1 for k, v in ops.launch_counts(sequence=True).items()}
    assert set(ops.launches_since(before)) == set(plain + SEQ_COUNTERS)        # launches_since sees the range
    first = 256
    assert [lib.ptgnn_amd_launch_name(first + i) for i in range(4)] == [n.encode() for n in SEQ_COUNTERS] + [None]
    assert lib.ptgnn_amd_launch_name(first + 3) is None
    assert lib.ptgnn_amd_launch_count(first) == ops.launch_counts(sequence=True)["vocab_loss"]
    assert lib.ptgnn_amd_launch_count(first + 3) == -1
    for end in (13, 64 + 17, 128 + 4, 192 + 4):                      # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(end) is None and lib.ptgnn_amd_launch_name(end - 1) is not None


def test_workspaces_and_argument_checks_without_a_gpu(lib):
    assert lib.ptgnn_amd_vocab_loss_workspace_bytes(0, 5) == 0
    assert lib.ptgnn_amd_vocab_loss_backward_workspace_bytes(0, 5) == 0
    assert lib.ptgnn_amd_copy_loss_finish_workspace_bytes(0) == 0
    for rows, vocab in ((1, 1), (7, 23), (448, 20000)):
        assert lib.ptgnn_amd_vocab_loss_workspace_bytes(rows, vocab) >= rows * 12
        assert lib.ptgnn_amd_vocab_loss_backward_workspace_bytes(rows, vocab) >= (rows + 7) // 8 * vocab * 4
    assert lib.ptgnn_amd_copy_loss_finish_workspace_bytes(5) == 20
    fake = ctypes.c_void_p(4096)                                      # never dereferenced: every call fails its checks first

    def fwd(scores=fake, ld=23, rows=5, vocab=23, norm=fake, picked=fake, stats=fake, ws=fake, ws_bytes=1 << 20):
        return lib.ptgnn_amd_vocab_loss_f32(scores, ld, rows, vocab, fake, fake, fake, norm, picked, stats, ws, ws_bytes,
                                            None)

    for bad in (dict(rows=-1), dict(ld=22), dict(vocab=0), dict(vocab=-3, ld=0), dict(scores=None), dict(norm=None),
                dict(picked=None), dict(stats=None), dict(stats=ctypes.c_void_p(4100))):
        assert fwd(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"vocab_loss:"), bad
    assert fwd(vocab=2 ** 31 - 1, ld=2 ** 31 - 1) == -2 and lib.ptgnn_amd_last_error().startswith(b"vocab_loss:")
    assert fwd(ws_bytes=8) == -4 and lib.ptgnn_amd_last_error().startswith(b"vocab_loss:")
    assert fwd(ws=None) == -4
    assert fwd(rows=0, scores=None, norm=None, picked=None, stats=None, ws=None, ws_bytes=0) == 0     # nothing to do

    def bwd(scores=fake, ld=23, rows=9, vocab=23, stats=fake, grad=fake, ld_g=23, grad_bias=fake, ws=fake, ws_bytes=1 << 20):
        return lib.ptgnn_amd_vocab_loss_backward_f32(scores, ld, rows, vocab, fake, fake, fake, stats, fake, fake, grad, ld_g,
                                                     fake, grad_bias, ws, ws_bytes, None)

    for bad in (dict(rows=-1), dict(ld=22), dict(ld_g=22), dict(vocab=0), dict(scores=None), dict(stats=None),
                dict(grad=None)):
        assert bwd(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"vocab_loss_backward:"), bad
    assert bwd(ws_bytes=2 * 24 * 4 - 1) == -4 and lib.ptgnn_amd_last_error().startswith(b"vocab_loss_backward:")
    assert bwd(ws=None) == -4
    assert bwd(rows=0) == 0

    def finish(gen=fake, samples=4, steps=5, loss=fake, ws=fake, ws_bytes=1 << 10):
        return lib.ptgnn_amd_copy_loss_finish_f32(gen, fake, fake, fake, 1, fake, samples, steps, loss, fake, fake, ws,
                                                  ws_bytes, None)

    for bad in (dict(samples=-1), dict(steps=-1), dict(gen=None), dict(loss=None)):
        assert finish(**bad) == -1 and lib.ptgnn_amd_last_error().startswith(b"copy_loss_finish:"), bad
    assert finish(samples=2 ** 30, steps=8) == -2 and lib.ptgnn_amd_last_error().startswith(b"copy_loss_finish:")
    assert finish(ws_bytes=15) == -4 and lib.ptgnn_amd_last_error().startswith(b"copy_loss_finish:")
    assert finish(samples=0) == 0 and finish(steps=0) == 0


def test_wrappers_refuse_host_tensors():
    from ptgnn_amd import _lib, ops
    scores, idx = torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.vocab_loss(scores, None, None, idx)
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.vocab_loss_backward(scores, None, None, idx, torch.zeros(3, 2), None, None)
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.copy_loss_finish(torch.zeros(1, 3), torch.zeros(1, 3), None, idx.reshape(1, 3), 1, idx[:1])
