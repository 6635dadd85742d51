"""GruCopyingDecoder on host tensors (ptgnn_amd.sequence, the reference's operator order on torch and the facade's CPU
route) against fixtures of the reference's own class (tests/golden/make_golden_decoder.py): state_dict keys, same-seed
initial parameters, the loss, the three outputs of `_compute_logprobs` and every gradient; plus the C ABI of
csrc/segment_scores.hip as far as it goes without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from decoder_cases import CASES, UNK_ID, build, inputs_of, load, ref_loss, state_of, weights_of
from ptgnn_amd import sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_TOL = 2e-5          # the bar of tests/test_gpu_attention_pool.py, relative to max(1, max |want|)
IDS = [name for name, _ in CASES]
SYMBOLS = ["ptgnn_amd_segment_scores_backward_f32", "ptgnn_amd_segment_scores_backward_workspace_bytes",
           "ptgnn_amd_segment_scores_f32", "ptgnn_amd_segment_scores_supported",
           "ptgnn_amd_segment_scores_workspace_bytes"]


def close(got, want, tol=FIXTURE_TOL):
    """Finite entries within tol * max(1, max |want|), -inf entries at the same positions."""
    got, want = got.detach().double(), torch.as_tensor(want).double()
    if got.shape != want.shape or not torch.equal(got == -np.inf, want == -np.inf):
        return False
    finite = torch.isfinite(want)
    if not bool(finite.any()):
        return True
    scale = max(1.0, float(want[finite].abs().max()))
    return float((got[finite] - want[finite]).abs().max()) <= tol * scale


def test_fixtures_hold_the_cases_they_are_meant_to():
    for name, spec in CASES:
        fx = load(name)
        assert json.loads(str(fx["spec"])) == spec
        B, L = spec["B"], spec["T"] - 1
        idx = fx["input_memories_origin_idx"]
        counts = np.bincount(idx, minlength=B)
        assert counts.tolist() == spec["sizes"] and 0 in counts[1:-1].tolist() and counts[-1] > 0
        assert not bool((idx[1:] >= idx[:-1]).all())                                   # shuffled map
        tokens, where = fx["target_token_ids"], fx["copyable_elements_sample_idxs"]
        per_location = np.bincount(where, minlength=B * L)
        assert tokens[0, 1] == UNK_ID and per_location[0] >= 2                          # UNK with a valid copy, 2 entries
        assert tokens[B - 1, 1] == UNK_ID and per_location[(B - 1) * L] == 0            # UNK that must be generated
        assert (per_location == 0).any()
        assert (idx[fx["copyable_elements_idxs"] // L] == where // L).all()             # a sample copies its own memories
        assert L == 1 or (fx["target_lengths"] < L).any()
        assert np.isfinite(fx["loss"]) and (fx["copy_logprobs"].shape, fx["target_logprobs"].shape,
                                            fx["gru_state"].shape) == ((len(idx), L), (B, L, spec["V"]), (1, B, spec["H"]))
    assert {s["T"] - 1 for _, s in CASES} >= {1, 7} and any(s["Dm"] % 4 for _, s in CASES)


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_state_dict_keys_and_same_seed_initial_parameters_match_the_reference(name, spec):
    want = state_of(load(name))
    torch.manual_seed(spec["seed"])
    module = build(spec, sequence)
    assert list(module.state_dict()) == list(want)               # mangled names, creation order
    p = "_GruCopyingDecoder__"
    assert list(want) == [p + "hidden_to_vocab", p + "vocab_bias", p + "embedding_layer.weight",
                          p + "output_gru.weight_ih_l0", p + "output_gru.weight_hh_l0", p + "output_gru.bias_ih_l0",
                          p + "output_gru.bias_hh_l0", p + "memories_to_standard_attention.weight",
                          p + "memories_to_copy_attention.weight"]
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k
    build(spec, sequence).load_state_dict(want, strict=True)


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_reproduces_the_reference(name, spec):
    fx = load(name)
    module = build(spec, sequence)
    module.load_state_dict(state_of(fx), strict=True)
    inputs = inputs_of(fx)
    inputs["input_memories"].requires_grad_(True)
    inputs["initial_states"].requires_grad_(True)
    with torch.no_grad():
        outs = module._compute_logprobs(inputs["initial_states"], inputs["input_memories"],
                                        inputs["input_memories_origin_idx"], inputs["target_token_ids"][:, :-1])
    for got, key in zip(outs, ("copy_logprobs", "target_logprobs", "gru_state")):
        assert not got.is_cuda and close(got, fx[key]), key
    loss = module(**inputs)
    assert close(loss, fx["loss"])
    loss.backward()
    assert close(inputs["input_memories"].grad, fx["grad.input_memories"])
    assert close(inputs["initial_states"].grad, fx["grad.initial_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k


def test_the_restatement_of_the_gpu_tests_agrees_with_the_reference_fixtures():
    """tests/decoder_cases.ref_loss is the float64 yardstick of tests/test_gpu_decoder.py: pinned to the reference here."""
    for name, spec in CASES[:3]:
        fx = load(name)
        module = build(spec, sequence)
        module.load_state_dict(state_of(fx), strict=True)
        w = weights_of(module, torch.float64)
        inputs = inputs_of(fx, lambda t: t.double() if t.is_floating_point() else t)
        inputs["input_memories"].requires_grad_(True)
        loss = ref_loss(w, **inputs)
        loss.backward()
        assert close(loss, fx["loss"]) and close(inputs["input_memories"].grad, fx["grad.input_memories"])
        for k, p in module.named_parameters():
            assert close(w[k.split("__", 1)[1]].grad, fx["grad." + k]), k


def test_memoryless_samples_get_minus_infinity_and_half_inputs_return_their_dtype():
    name, spec = CASES[0]
    fx = load(name)
    module = build(spec, sequence)
    module.load_state_dict(state_of(fx), strict=True)
    inp = inputs_of(fx)
    with torch.no_grad():
        copy32, target32, state32 = module._compute_logprobs(
            inp["initial_states"], inp["input_memories"].bfloat16().float(), inp["input_memories_origin_idx"],
            inp["target_token_ids"][:, :-1])
        copy16, target16, state16 = module._compute_logprobs(
            inp["initial_states"], inp["input_memories"].bfloat16(), inp["input_memories_origin_idx"],
            inp["target_token_ids"][:, :-1])
    assert copy16.dtype == target16.dtype == torch.bfloat16 and state16.dtype == torch.float32
    assert torch.equal(copy16, copy32.bfloat16()) and torch.equal(target16, target32.bfloat16())
    # the memory-less sample normalises over the vocabulary alone
    empty = spec["sizes"].index(0)
    assert float(torch.logsumexp(target32[empty], dim=-1).abs().max()) <= 1e-5


def test_exported_from_the_package_and_refuses_the_sharded_form():
    import ptgnn_amd
    assert ptgnn_amd.GruCopyingDecoder is sequence.GruCopyingDecoder
    with pytest.raises(ptgnn_amd.PtgnnAmdError, match="cannot combine partial pools"):
        build(CASES[0][1], sequence).forward_sharded()


def test_gru_cell_keeps_its_behaviour_and_delegates_to_the_weights_form():
    from ptgnn_amd import dense
    cell = torch.nn.GRUCell(4, 4)
    with pytest.raises(ptgnn_amd_error(), match="dense.gru_cell needs 2-D float32 CUDA matrices"):
        dense.gru_cell(cell, torch.randn(3, 4), torch.randn(3, 4))
    with pytest.raises(ptgnn_amd_error(), match="dense.gru_cell needs 2-D float32 CUDA matrices"):
        dense.gru_cell_weights(torch.randn(3, 4), torch.randn(3, 4), cell.weight_ih, cell.weight_hh, cell.bias_ih,
                               cell.bias_hh)


def ptgnn_amd_error():
    from ptgnn_amd import PtgnnAmdError
    return PtgnnAmdError


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_declares_the_five_symbols_and_lib_binds_them(lib):
    from ptgnn_amd import _lib, build as B
    assert "segment_scores.hip" in B.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_segment_scores[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "segment_scores" in s) == declared


def test_library_still_reports_version_102_and_names_the_two_counters(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    counts = ops.launch_counts(aggregation=True)
    assert "segment_scores" in counts and "segment_scores_backward" in counts
    assert "segment_scores" not in ops.launch_counts()


def test_supported_range_and_argument_checks_without_a_gpu(lib):
    from ptgnn_amd import _lib
    sup = lib.ptgnn_amd_segment_scores_supported
    assert [sup(k, 1) for k in (0, 1, 128, 1024, 1025)] == [0, 1, 1, 1, 0]
    assert [sup(128, l) for l in (0, 1, 7, 8, 9)] == [0, 1, 1, 1, 0]
    assert lib.ptgnn_amd_segment_scores_workspace_bytes(5, 1000, 128, 7) > 0
    assert lib.ptgnn_amd_segment_scores_backward_workspace_bytes(5, 1000, 128, 7) >= (1000 // 128 + 5) * 7 * 128 * 4
    for dim, vectors in ((128, 9), (1025, 7)):
        rc = lib.ptgnn_amd_segment_scores_f32(None, dim, None, None, None, 3, 10, dim, vectors, None, None, None, 0, None)
        assert rc == _lib.EUNSUPPORTED and b"segment_scores" in lib.ptgnn_amd_last_error()
        rc = lib.ptgnn_amd_segment_scores_backward_f32(None, dim, None, None, None, 3, 10, dim, vectors, None, None, None,
                                                       None, None, dim, None, None, 0, None)
        assert rc == _lib.EUNSUPPORTED and b"segment_scores_backward" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_segment_scores_f32(None, 128, None, None, None, 3, 10, 128, 7, None, None, None, 0, None)
    assert rc == -1 and b"segment_scores" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_segment_scores_f32(None, 128, None, None, None, -1, 10, 128, 7, None, None, None, 0, None)
    assert rc == -1
