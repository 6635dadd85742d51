"""TokenUnitEmbedder / SubtokenUnitEmbedder on host tensors (ptgnn_amd.embeddings, the reference's operator order on
torch) against fixtures of the reference's own classes (tests/golden/make_golden_embedder.py): state_dict keys, same-seed
initial parameters, the output bit for bit and every gradient; plus the C ABI of csrc/embedding_bag.hip as far as it goes
without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from embedder_cases import CASES, args_of, build, load, loss_of, ref_pool, state_of
from ptgnn_amd import embeddings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-5             # gradients to 2e-5 of the largest reference entry
IDS = [name for name, _ in CASES]
SYMBOLS = ["ptgnn_amd_embedding_bag_backward_f32", "ptgnn_amd_embedding_bag_backward_workspace_bytes",
           "ptgnn_amd_embedding_bag_f32", "ptgnn_amd_embedding_bag_keys", "ptgnn_amd_embedding_bag_supported"]
DEFAULT_COUNTERS = ["k_stream_linear", "k_stream_linear_ring", "k_stream_gru", "k_stream_gru_ring", "k_stream_edge",
                    "k_stream_edge_shared", "k_stream_edge_v2", "k_wgrad_stream", "k_linear_tlp", "k_gru", "k_edge_linear",
                    "k_edge_wgrad", "k_gather_update"]


def test_fixtures_hold_the_cases_they_are_meant_to():
    kinds = set()
    for name, spec in CASES:
        fx = load(name)
        assert json.loads(str(fx["spec"])) == spec
        assert fx["out"].shape == (spec["B"], spec["D"]) and fx["token_idxs"].dtype == np.int64
        kinds.add((spec["kind"], spec["D"], spec["dense"]))
        if spec["kind"] == "token":
            continue
        ids, lengths, S = fx["token_idxs"], fx["lengths"], spec["S"]
        assert ids.shape == (spec["B"], S) and lengths.dtype == np.int64
        assert ids[0, 0] == ids[0, 1] and lengths[0] >= 2                      # one id in two live slots
        assert {1, S, S + 2} <= set(lengths.tolist())
        assert (0 in lengths.tolist()) == spec["zero"]
        assert ids.max() < spec["V"] - 3                                        # vocabulary rows nobody references
        assert not fx["grad._SubtokenUnitEmbedder__embeddings.weight"][-3:].any()
        if spec["kind"] == "max" and not spec["dense"]:
            assert np.isneginf(fx["out"][lengths == 0]).all() and np.isfinite(fx["out"][lengths > 0]).all()
        else:
            assert np.isfinite(fx["out"]).all()
    assert kinds >= {(k, d, True) for k in ("sum", "mean", "max") for d in (64, 128)} | {("max", 64, False),
                                                                                         ("token", 64, False)}


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_state_dict_keys_and_same_seed_initial_parameters_match_the_reference(name, spec):
    want = state_of(load(name))
    torch.manual_seed(spec["seed"])
    module = build(spec, embeddings)
    assert list(module.state_dict()) == list(want)               # mangled names, creation order
    cls = "_TokenUnitEmbedder__" if spec["kind"] == "token" else "_SubtokenUnitEmbedder__"
    assert list(want) == [cls + "embeddings.weight"] + ([cls + "out_layer.weight"] if spec["dense"] else [])
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k
    build(spec, embeddings).load_state_dict(want, strict=True)
    assert module.embedding_layer.weight is dict(module.named_parameters())[cls + "embeddings.weight"]


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_reproduces_the_reference(name, spec):
    fx = load(name)
    module = build(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    args, coef = args_of(fx), torch.from_numpy(fx["coef"])
    out = module(*args)
    assert not out.is_cuda and torch.equal(out.detach(), torch.from_numpy(fx["out"]))        # bit for bit
    loss_of(out, args, coef).backward()
    for k, p in module.named_parameters():
        want = torch.from_numpy(fx["grad." + k])
        assert float((p.grad - want).abs().max()) <= GRAD_TOL * float(want.abs().max()), k


def test_the_restatement_of_the_gpu_tests_agrees_with_the_reference_fixtures():
    """tests/embedder_cases.ref_pool is the yardstick of tests/test_gpu_embedder.py: pinned to the reference here."""
    for name, spec in CASES:
        if spec["kind"] == "token":
            continue
        fx = load(name)
        state = state_of(fx)
        table = state["_SubtokenUnitEmbedder__embeddings.weight"]
        ids, lengths = args_of(fx)
        pooled = ref_pool(table, ids, lengths, spec["kind"])
        if spec["dense"]:
            pooled = torch.nn.functional.linear(pooled, state["_SubtokenUnitEmbedder__out_layer.weight"])
        want = torch.from_numpy(fx["out"])
        finite = torch.isfinite(want)
        assert torch.equal(torch.isfinite(pooled), finite)
        assert float((pooled[finite] - want[finite]).abs().max()) <= 2e-5 * max(1.0, float(want[finite].abs().max()))


def test_exported_from_the_package():
    import ptgnn_amd
    assert ptgnn_amd.TokenUnitEmbedder is embeddings.TokenUnitEmbedder
    assert ptgnn_amd.SubtokenUnitEmbedder is embeddings.SubtokenUnitEmbedder
    from ptgnn_amd import sequence
    assert embeddings._rows is sequence._rows                    # one row gather with autograd, shared


def test_cpu_tensors_never_load_the_library(monkeypatch):
    from ptgnn_amd import _lib

    def refuse():
        raise AssertionError("a CPU forward / backward loaded the library")

    monkeypatch.setattr(_lib, "load", refuse)
    for kind in ("sum", "mean", "max"):
        module = embeddings.SubtokenUnitEmbedder(20, 8, 0.0, kind)
        module(torch.randint(0, 20, (6, 3)), torch.tensor([1, 2, 3, 3, 1, 2])).sum().backward()
    embeddings.TokenUnitEmbedder(20, 8, 0.1)(torch.randint(0, 20, (6,))).sum().backward()


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_declares_the_new_symbols_and_lib_binds_them(lib):
    from ptgnn_amd import _lib, build as B
    assert "embedding_bag.hip" in B.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_embedding_bag[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "embedding_bag" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))


def test_library_still_reports_version_102_and_the_default_counter_list_is_unchanged(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    assert list(ops.launch_counts()) == DEFAULT_COUNTERS
    counts = ops.launch_counts(aggregation=True)
    assert "embedding_bag" in counts and "embedding_bag_backward" in counts
    assert list(counts)[-2:] == ["embedding_bag", "embedding_bag_backward"]


def test_supported_range(lib):
    sup = lib.ptgnn_amd_embedding_bag_supported
    for dim in (0, 3, 4, 6, 128, 1024, 1028):
        for slots in (0, 1, 32, 33):
            want = int(dim % 4 == 0 and 4 <= dim <= 1024 and 1 <= slots <= 32)
            assert sup(dim, slots) == want, (dim, slots)


def test_argument_checks_without_a_gpu(lib):
    from ptgnn_amd import _lib

    def forward(dim, slots, bags=3, vocab=10, mode=0):
        return lib.ptgnn_amd_embedding_bag_f32(None, dim, vocab, None, None, bags, slots, dim, mode, None, dim, None, None)

    def backward(dim, slots, bags=3, vocab=10, mode=0):
        return lib.ptgnn_amd_embedding_bag_backward_f32(None, dim, None, None, bags, slots, vocab, dim, mode, None, None,
                                                        None, None, dim, 0, None, None, None, 0, None, None, 0, None)

    for dim, slots in ((127, 5), (1028, 5), (128, 33)):
        assert forward(dim, slots) == _lib.EUNSUPPORTED and b"embedding_bag" in lib.ptgnn_amd_last_error()
        assert backward(dim, slots) == _lib.EUNSUPPORTED and b"embedding_bag_backward" in lib.ptgnn_amd_last_error()
    assert lib.ptgnn_amd_embedding_bag_keys(None, None, 3, 33, 10, None, None, None) == _lib.EUNSUPPORTED
    assert b"embedding_bag" in lib.ptgnn_amd_last_error()
    # null pointers, negative sizes, an unknown mode
    assert forward(128, 5) == -1 and b"embedding_bag" in lib.ptgnn_amd_last_error()
    assert backward(128, 5) == -1 and b"embedding_bag_backward" in lib.ptgnn_amd_last_error()
    assert forward(128, 5, bags=-1) == -1 and backward(128, 5, vocab=-1) == -1
    assert forward(128, 5, mode=3) == -1 and backward(128, 5, mode=-1) == -1
    assert lib.ptgnn_amd_embedding_bag_keys(None, None, 3, 5, 10, None, None, None) == -1
    assert lib.ptgnn_amd_embedding_bag_keys(None, None, -3, 5, 10, None, None, None) == -1
    # nothing to do: no bags
    assert forward(128, 5, bags=0) == 0
    wsb = lib.ptgnn_amd_embedding_bag_backward_workspace_bytes
    assert [wsb(7, 5, 128, m) for m in (0, 1, 2)] == [0, 7 * 128 * 4, 7 * 5 * 4]


def test_ops_wrappers_refuse_host_tensors():
    from ptgnn_amd import PtgnnAmdError, ops
    table, ids, lengths = torch.randn(10, 8), torch.zeros(3, 2, dtype=torch.int64), torch.ones(3, dtype=torch.int64)
    with pytest.raises(PtgnnAmdError, match="must live on the GPU"):
        ops.embedding_bag(table, ids, lengths, "sum")
    with pytest.raises(PtgnnAmdError, match="must live on the GPU"):
        ops.embedding_bag_backward(torch.randn(3, 8), ids, lengths, "sum", 10)
