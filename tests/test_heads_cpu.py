"""The task heads (ptgnn_amd.heads) and LinearFeatureEmbedder without a GPU: the fixtures' input conditions, the reference's
state_dict keys and same-seed initial parameters, the CPU route against the reference fixtures, and the C ABI of
csrc/task_heads.hip as far as it goes without a device."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import ptgnn_amd
from head_cases import (ALL_HEAD_CASES, LFE_CASES, build, build_lfe, call_args, conditions_hold, inputs_of, load,
                        make_inputs, state_of)
from ptgnn_amd import embeddings, heads
from ptgnn_amd.gnn import GnnOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_TOL = 2e-5          # the bar of tests/test_decoder_cpu.py, relative to max(1, max |want|)
IDS = [name for _, name, _ in ALL_HEAD_CASES]
SYMBOLS = sorted(["ptgnn_amd_logit_loss_workspace_bytes", "ptgnn_amd_logit_loss_f32", "ptgnn_amd_logit_loss_backward_f32",
                  "ptgnn_amd_candidate_scores_supported", "ptgnn_amd_candidate_scores_workspace_bytes",
                  "ptgnn_amd_candidate_scores_f32", "ptgnn_amd_candidate_scores_backward_workspace_bytes",
                  "ptgnn_amd_candidate_scores_backward_f32"])
HEAD_COUNTERS = ["logit_loss", "logit_loss_backward", "candidate_scores", "candidate_scores_backward"]
COUNT_METRICS = ("Accuracy",)           # ratios of two integer counts: compared exactly


def close(got, want, tol=FIXTURE_TOL):
    got, want = torch.as_tensor(got).detach().double(), torch.as_tensor(want).double()
    if got.shape != want.shape:
        return False
    err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"    |got - want| = {err:.3e} (scale {scale:.3e})")
    return err <= tol * scale


def fixture_module(kind, name, spec):
    fx = load(name)
    module = build(kind, spec, heads, GnnOutput)
    module.load_state_dict(state_of(fx), strict=True)
    return fx, module


@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_fixture_inputs_meet_the_input_conditions(kind, name, spec):
    fx = load(name)
    assert conditions_hold(kind, fx)
    inputs = make_inputs(kind, spec, torch.Generator().manual_seed(9000 + spec["seed"]))
    for k, v in inputs.items():                                       # the fixture holds the inputs of its case
        assert torch.equal(torch.from_numpy(fx[k]), v), k
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 700_000 for name in IDS)


@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_state_dict_keys_initial_parameters_and_strict_load(kind, name, spec):
    fx = load(name)
    torch.manual_seed(spec["seed"])
    module = build(kind, spec, heads, GnnOutput)
    want = state_of(fx)
    assert list(module.state_dict()) == list(want)                    # the reference's name-mangled keys, in its order
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k                             # same seed, same draws in the same order
    other = build(kind, spec, heads, GnnOutput)
    other.load_state_dict(want, strict=True)                          # reference -> ptgnn_amd
    assert set(other.state_dict()) == set(want)                       # ptgnn_amd -> reference: the same key set


def test_reference_attribute_names():
    g2c = build("g2c", dict(D=4, C=3), heads, GnnOutput)
    assert list(g2c.state_dict()) == ["_Graph2ClassModule__node_to_class.weight", "_Graph2ClassModule__node_to_class.bias"]
    assert isinstance(g2c._Graph2ClassModule__loss, nn.CrossEntropyLoss)
    vm = build("vm", dict(H=4), heads, GnnOutput)
    assert list(vm.state_dict()) == ["_VarMisuseGraphModel__candidate_scores.weight"]
    assert vm._gnn.output_node_state_dim == 4                         # a single underscore in the reference
    ppi = build("ppi", dict(D=4, C=3), heads, GnnOutput)
    assert list(ppi.state_dict()) == ["_PPIClassification__output_representation_to_logits.weight",
                                      "_PPIClassification__output_representation_to_logits.bias"]
    for module in (g2c, vm, ppi):
        assert isinstance(module, ptgnn_amd.gnn.ModuleWithMetrics)


@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_cpu_route_against_the_reference_fixture(kind, name, spec):
    fx, module = fixture_module(kind, name, spec)
    inputs = inputs_of(fx)
    if kind == "g2c":
        probs, classes, graph_idx = module.predict(call_args(kind, inputs)[0])
        assert close(probs, fx["predict.probs"])
        assert torch.equal(classes, torch.from_numpy(fx["predict.classes"]))
        assert torch.equal(graph_idx, torch.from_numpy(fx["predict.graph_idx"]))
    module.reset_metrics()
    states = inputs["node_states"].clone().requires_grad_(True)
    loss = module(*call_args(kind, inputs, states=states))
    loss.backward()
    assert close(loss, fx["loss"])
    assert close(states.grad, fx["grad.node_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k
    first = module.report_metrics()
    with torch.no_grad():
        assert close(module(*call_args(kind, inputs, second=True)), fx["second.loss"])
    second = module.report_metrics()
    for tag, got in (("metrics1.", first), ("metrics2.", second)):
        assert sorted(tag + k for k in got) == sorted(k for k in fx if k.startswith(tag))
        for k, v in got.items():
            if k in COUNT_METRICS:
                assert float(v) == float(fx[tag + k]), (tag, k)
            else:
                assert close(float(v), fx[tag + k]), (tag, k)
    module.reset_metrics()                                            # a working reset: the first minibatch alone again
    with torch.no_grad():
        module(*call_args(kind, inputs))
    for k, v in module.report_metrics().items():
        assert close(float(v), fx["metrics1." + k]), k


def test_metric_names():
    names = {"g2c": ["Accuracy"], "vm": ["Accuracy"], "ppi": ["f1_score", "pr_score", "re_score"]}
    for kind, name, spec in ALL_HEAD_CASES:
        assert sorted(k[len("metrics1."):] for k in load(name) if k.startswith("metrics1.")) == names[kind]


def test_cpu_tensors_never_load_the_library(monkeypatch):
    from ptgnn_amd import _lib

    def refuse():
        raise AssertionError("a CPU forward / backward loaded the library")

    monkeypatch.setattr(_lib, "load", refuse)
    for kind, name, spec in ALL_HEAD_CASES[::4]:
        fx, module = fixture_module(kind, name, spec)
        module(*call_args(kind, inputs_of(fx))).backward()
        module.report_metrics()
    embeddings.LinearFeatureEmbedder(5, 4, nn.Tanh())(torch.randn(3, 5)).sum().backward()


@pytest.mark.parametrize("name,spec", LFE_CASES, ids=[n for n, _ in LFE_CASES])
def test_linear_feature_embedder_against_its_fixture(name, spec):
    fx = load(name)
    torch.manual_seed(spec["seed"])
    module = build_lfe(spec, embeddings)
    want = state_of(fx)
    assert list(module.state_dict()) == ["_LinearFeatureEmbedder__linear_map.weight"] == list(want)
    assert torch.equal(module.state_dict()["_LinearFeatureEmbedder__linear_map.weight"],
                       want["_LinearFeatureEmbedder__linear_map.weight"])
    children = dict(module.named_children())                          # the activation registered as the reference does
    assert ("_LinearFeatureEmbedder__activation" in children) == (spec["act"] is not None)
    x = torch.from_numpy(fx["features"]).clone().requires_grad_(True)
    out = module(x)
    (out * torch.from_numpy(fx["cotangent"])).sum().backward()
    assert close(out, fx["out"]) and close(x.grad, fx["grad.features"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k


def test_package_exports():
    for name in ("Graph2ClassModule", "VarMisuseGraphModel", "PPIClassification"):
        assert getattr(ptgnn_amd, name) is getattr(heads, name)
    assert ptgnn_amd.LinearFeatureEmbedder is embeddings.LinearFeatureEmbedder


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_exports_map_and_ctypes_agree_on_the_new_symbols(lib):
    from ptgnn_amd import _lib, build as B
    assert "task_heads.hip" in B.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_(?:logit_loss|candidate_scores)[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    assert "global: ptgnn_amd_*;" in open(os.path.join(ROOT, "ptgnn_amd", "csrc", "exports.map")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "logit_loss" in s or "candidate_scores" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))


def test_head_counters_have_their_own_keyword(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    plain = list(ops.launch_counts())
    assert not set(HEAD_COUNTERS) & set(ops.launch_counts(aggregation=True, char_cnn=True))
    assert list(ops.launch_counts(heads=True)) == plain + HEAD_COUNTERS
    before = {k: v - 1 for k, v in ops.launch_counts(heads=True).items()}
    assert set(ops.launches_since(before)) == set(plain + HEAD_COUNTERS)       # launches_since sees the range
    first = 192
    assert [lib.ptgnn_amd_launch_name(first + i) for i in range(5)] == [n.encode() for n in HEAD_COUNTERS] + [None]
    assert lib.ptgnn_amd_launch_count(first) == ops.launch_counts(heads=True)["logit_loss"]
    assert lib.ptgnn_amd_launch_count(first + 4) == -1


def test_supported_range_workspaces_and_argument_checks_without_a_gpu(lib):
    from ptgnn_amd import _lib
    sup = lib.ptgnn_amd_candidate_scores_supported
    for dim in (0, 2, 4, 6, 8, 60, 128, 1024, 1026, 1028):
        assert sup(dim) == int(dim % 4 == 0 and 4 <= dim <= 1024), dim
    assert [lib.ptgnn_amd_logit_loss_workspace_bytes(r) for r in (0, 1, 128, 129)] == [0, 32, 32, 64]
    assert [lib.ptgnn_amd_candidate_scores_workspace_bytes(g) for g in (0, 1, 7)] == [0, 4, 28]
    assert lib.ptgnn_amd_candidate_scores_backward_workspace_bytes(0, 8) == 0
    assert lib.ptgnn_amd_candidate_scores_backward_workspace_bytes(3, 8) == 3 * 16 * 4
    fake = ctypes.c_void_p(4096)                                      # never dereferenced: every call fails its checks first

    def loss(logits=fake, ld=7, rows=5, classes=7, mode=0, targets=fake, ld_t=7, lse=fake, out=fake, totals=fake, ws=fake,
             ws_bytes=1 << 20):
        return lib.ptgnn_amd_logit_loss_f32(logits, ld, rows, classes, mode, targets, ld_t, lse, None, None, None, out, totals,
                                            None, ws, ws_bytes, None)

    for bad in (dict(rows=-1), dict(classes=0), dict(mode=2), dict(logits=None), dict(ld=6), dict(lse=None), dict(out=None),
                dict(totals=None), dict(mode=1, targets=None), dict(mode=1, ld_t=6), dict(totals=ctypes.c_void_p(4100))):
        assert loss(**bad) == -1 and b"logit_loss" in lib.ptgnn_amd_last_error(), bad
    assert loss(ws_bytes=31) == -4 and loss(ws=None) == -4
    assert loss(rows=0, logits=None, targets=None, lse=None, out=None, totals=None, ws=None) == 0     # nothing to do

    def loss_bwd(rows=5, classes=7, mode=0, targets=fake, lse=fake, totals=fake, g=fake, grad=fake, ld_g=7):
        return lib.ptgnn_amd_logit_loss_backward_f32(fake, 7, rows, classes, mode, targets, 7, lse, totals, g, grad, ld_g, None)

    for bad in (dict(rows=-1), dict(mode=-1), dict(targets=None), dict(lse=None), dict(totals=None), dict(g=None),
                dict(grad=None), dict(ld_g=6)):
        assert loss_bwd(**bad) == -1 and b"logit_loss_backward" in lib.ptgnn_amd_last_error(), bad
    assert loss_bwd(rows=0) == 0

    def cand(x=fake, ld=8, nodes=10, cn=6, g=2, dim=8, w=fake, correct=fake, out=fake, totals=fake, ws=fake, ws_bytes=1 << 20):
        return lib.ptgnn_amd_candidate_scores_f32(x, ld, nodes, fake, fake, fake, fake, fake, cn, g, dim, w, correct, fake,
                                                  fake, fake, out, totals, None, ws, ws_bytes, None)

    for bad in (dict(nodes=-1), dict(cn=-1), dict(g=-1), dict(dim=0), dict(x=None), dict(w=None), dict(ld=4), dict(out=None),
                dict(totals=None), dict(nodes=0)):
        assert cand(**bad) == -1 and b"candidate_scores" in lib.ptgnn_amd_last_error(), bad
    for dim in (6, 1028):
        assert cand(dim=dim, ld=dim) == _lib.EUNSUPPORTED and b"candidate_scores" in lib.ptgnn_amd_last_error()
    assert cand(ws_bytes=7) == -4 and cand(g=0) == 0


def test_wrappers_refuse_host_tensors():
    from ptgnn_amd import _lib, ops
    x, idx = torch.zeros(4, 8), torch.zeros(3, dtype=torch.int64)
    plan = None
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.logit_loss(torch.zeros(3, 5), idx, "softmax")
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.logit_loss_backward(torch.zeros(3, 5), idx, "softmax", torch.zeros(3), torch.zeros(8, dtype=torch.int64),
                                torch.ones(()))
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.candidate_scores(x, idx, idx[:1], idx, plan, torch.zeros(16))
    with pytest.raises(_lib.PtgnnAmdError, match="must live on the GPU"):
        ops.candidate_scores_backward(x, idx, idx[:1], idx, plan, torch.zeros(16), None, torch.zeros(3), torch.zeros(1),
                                      None)
