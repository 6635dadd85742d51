"""The score-free loss of the copying decoder without a GPU: the C ABI of csrc/projection_loss.hip as far as it goes
without a device, its launch counters, and GruCopyingDecoder.score_free_loss on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from decoder_cases import CASES, build, inputs_of, load, state_of
from ptgnn_amd import _lib, build as B, heads, ops, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = sorted("ptgnn_amd_projection_loss" + s for s in ("_supported", "_workspace_bytes", "_f32",
                                                           "_backward_workspace_bytes", "_backward_f32"))
COUNTERS = ["projection_loss", "projection_loss_backward"]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    assert "projection_loss.hip" in B.SOURCES
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_projection_loss[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS == sorted(s for s in _lib.SIGNATURES if "projection_loss" in s)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert hasattr(raw, s) and len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s
    assert "grucopydecoder.py:111-135, 178-181" in header
    assert [lib.ptgnn_amd_projection_loss_supported(e) for e in (0, 1, 256, 257)] == [0, 1, 1, 0]
    assert lib.ptgnn_amd_projection_loss_workspace_bytes(0, 5) == 0
    assert lib.ptgnn_amd_projection_loss_backward_workspace_bytes(448, 20000, 256) == 4 * 20 * 448 * 256


def test_the_counters_have_their_own_keyword(lib):
    assert lib.ptgnn_amd_version() == 102
    plain = list(ops.launch_counts())
    others = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True, beam=True,
                               half=True, edge16=True, half_training=True, edge16_dst=True, beam_finish=True,
                               attention16=True, attention16_training=True, edge16_training=True)
    assert not set(COUNTERS) & set(others)
    assert list(ops.launch_counts(projection_loss=True)) == plain + COUNTERS
    before = {k: v - 1 for k, v in ops.launch_counts(projection_loss=True).items()}
    assert set(ops.launches_since(before)) == set(plain + COUNTERS)     # launches_since sees the range
    assert [lib.ptgnn_amd_launch_name(960 + i) for i in range(3)] == [n.encode() for n in COUNTERS] + [None]
    assert lib.ptgnn_amd_launch_count(962) == -1
    for end in (13, 64 + 17, 128 + 4, 192 + 4, 256 + 3, 320 + 1, 384 + 1, 448 + 2, 512 + 2, 576 + 3, 640 + 1, 704 + 2,
                768 + 1, 832 + 2, 896 + 2):                             # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(end) is None and lib.ptgnn_amd_launch_name(end - 1) is not None


def test_score_free_loss_on_cpu_tensors_is_forward_and_the_switch_is_off():
    assert heads.Graph2SeqModule.use_score_free_loss is False and heads.Graph2SeqModule.use_fused_loss is True
    fx = load(CASES[0][0])
    module = build(CASES[0][1], sequence)
    module.load_state_dict(state_of(fx), strict=True)
    runs, threads = [], torch.get_num_threads()
    torch.set_num_threads(1)                                            # threaded CPU scatter-adds fold in no fixed order
    try:
        for fn in (module.forward, module.score_free_loss):
            module.zero_grad(set_to_none=True)
            loss = fn(**inputs_of(fx))
            loss.backward()
            runs.append([loss.detach()] + [p.grad.clone() for p in module.parameters()])
    finally:
        torch.set_num_threads(threads)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
