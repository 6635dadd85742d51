"""The 16-bit attention training step without a GPU: the `set_attention_training` switch of ptgnn_amd/precision.py, the
C ABI of ptgnn_amd_selfatt_train16_* as far as it goes without a device, and the precondition of every case of
tests/test_gpu_attention_training.py: from the two float64 references alone, the exact gradients lie at least twice
outside the derived bound around the rounded ones, so the GPU test cannot pass on the fp32 route."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import attention_training_cases as T
import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ptgnn_amd_selfatt_train16_backward", "ptgnn_amd_selfatt_train16_forward", "ptgnn_amd_selfatt_train16_supported"]
FLAGS = ("edge_gemm", "training", "mlp", "attention", "edge_training")
EINVAL, EUNSUPPORTED = -1, -2


def test_switch_defaults_off_restores_and_is_independent_of_the_five_flags():
    import ptgnn_amd
    from ptgnn_amd import precision
    for name in ("set_attention_training", "attention_training", "attention_training_inputs"):
        assert getattr(ptgnn_amd, name) is getattr(precision, name)
    assert precision._attention_training is False
    assert ptgnn_amd.set_attention_training(True) is False and ptgnn_amd.set_attention_training(False) is True
    with ptgnn_amd.attention_training():
        with ptgnn_amd.attention_training(False):
            assert precision._attention_training is False
        for v in C.HALF:                                   # matrix_inputs neither reads, sets nor resets it
            with ptgnn_amd.matrix_inputs(v, **{f: True for f in FLAGS}):
                assert precision._attention_training is True
            ptgnn_amd.set_matrix_inputs(v)
            assert ptgnn_amd.set_matrix_inputs(torch.float32) is v and precision._attention_training is True
        assert all(getattr(precision, "_" + f) is False for f in FLAGS)       # and it sets none of the five
    with pytest.raises(RuntimeError, match="boom"):
        with ptgnn_amd.attention_training():
            raise RuntimeError("boom")
    assert precision._attention_training is False


def test_inputs_are_float32_on_cpu_tensors_and_follow_the_dtype_setting_otherwise(monkeypatch):
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu, gpu = torch.zeros(1), type("Fake", (), {"is_cuda": True})()       # the readers look at is_cuda only
    for v in C.HALF:
        with ptgnn_amd.matrix_inputs(v):
            assert precision.attention_training_inputs(gpu) is torch.float32          # switch off
            with ptgnn_amd.attention_training():
                assert precision.attention_training_inputs(gpu) is v
                assert precision.attention_training_inputs(cpu) is torch.float32      # CPU tensors: fp32 in training
                assert precision.attention_inputs(gpu) is torch.float32               # the inference flag stays off
        with ptgnn_amd.matrix_inputs("autocast"), ptgnn_amd.attention_training():
            assert precision.attention_training_inputs(gpu) is torch.float32          # no autocast region
            monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
            monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: v)
            assert precision.attention_training_inputs(gpu) is v and precision.attention_training_inputs(cpu) is torch.float32
            monkeypatch.undo()
    with ptgnn_amd.attention_training():
        assert precision.attention_training_inputs(gpu) is torch.float32              # float32 setting: fp32


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_counters_and_predicate_agree_on_the_new_entries(lib):
    from ptgnn_amd import _lib, build as B, ops, scatter
    assert "block_attention16_backward.hip" in B.SOURCES and lib.ptgnn_amd_version() == 102
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(ptgnn_amd_selfatt_[a-z0-9_]+)\s*\(", text))) == SYMBOLS
    assert sorted(s for s in _lib.SIGNATURES if "selfatt" in s) == SYMBOLS and "selfattmessagepassing.py:104-117" in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert hasattr(raw, s) and len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s
    names = [b"attention_train16", b"attention_train16_backward"]
    assert [lib.ptgnn_amd_launch_name(896 + i) for i in range(3)] == names + [None]
    assert lib.ptgnn_amd_launch_name(895) is None and lib.ptgnn_amd_launch_count(898) == -1
    for first, count in ((512, 2), (576, 3), (640, 1), (704, 2), (768, 1), (832, 2)):      # the earlier ranges end there
        assert lib.ptgnn_amd_launch_name(first + count) is None and lib.ptgnn_amd_launch_name(first + count - 1) is not None
    params = inspect.signature(ops.launch_counts).parameters
    assert params["attention16_training"].default is False and list(params)[-2:] == ["attention16_training", "edge16_training"]
    before = ops.launch_counts(attention16_training=True)
    assert list(before) == list(ops.launch_counts()) + [n.decode() for n in names]
    before["attention_train16_backward"] -= 1
    assert ops.launches_since(before) == {"attention_train16_backward": 1}      # launches_since reads the new range
    assert inspect.signature(ops.block_attention_backward).parameters["inputs"].default is None
    assert inspect.signature(scatter.block_attention).parameters["inputs"].default is None
    fn = lib.ptgnn_amd_selfatt_train16_supported
    for dt in (1, 2):
        assert all(fn(dk, dv, dt) == 1 for dk in (1, 17, 32, 128) for dv in (1, 6, 64, 128))
        assert not any(fn(dk, dv, dt) for dk, dv in ((0, 32), (32, 0), (129, 32), (32, 129), (-1, 1)))
    assert not any(fn(32, 32, dt) for dt in (0, 3, -1))
    assert ops.selfatt_train16_supported(17, 6, torch.float16) and not ops.selfatt_train16_supported(17, 6, torch.float32)


def test_entries_refuse_bad_arguments_before_anything_touches_the_device(lib):
    """The pointers are fake and never dereferenced: every call must answer from the argument checks."""
    p = 0x1000

    def forward(kqv=p, windows=p, out=p, lse=p, dk=32, dt=1, prob=0.25):
        return lib.ptgnn_amd_selfatt_train16_forward(kqv, 96, windows, 2, 10, 33, 1, dk, 32, out, 32, lse, dt, prob, 7, None)

    def backward(kqv=p, out=p, lse=p, go=p, windows=p, gkqv=p, ws=p, ws_bytes=1 << 20, dk=32, dt=1, prob=0.25):
        return lib.ptgnn_amd_selfatt_train16_backward(kqv, 96, out, 32, lse, go, 32, windows, 2, 10, 33, 1, dk, 32, prob, 7,
                                                      gkqv, 96, ws, ws_bytes, dt, None)

    def refused(rc, code, what, word):
        msg = lib.ptgnn_amd_last_error().decode()
        return rc == code and msg.startswith(what + ":") and word in msg

    for call, what, nulls in ((forward, "selfatt_train16_forward", ("kqv", "windows", "out", "lse")),
                              (backward, "selfatt_train16_backward", ("kqv", "out", "lse", "go", "windows", "gkqv"))):
        assert all(refused(call(**{name: None}), EINVAL, what, "null") for name in nulls)
        assert refused(call(dt=0), EINVAL, what, "dtype") and refused(call(dt=3), EINVAL, what, "dtype")
        assert refused(call(dk=129), EUNSUPPORTED, what, "129") and refused(call(prob=1.0), EINVAL, what, "dropout")
    assert backward(ws=None) < 0 and backward(ws_bytes=8) < 0


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_exact_gradients_lie_outside_the_derived_bound_of_the_rounded_ones(c, dt):
    ref = T.case(c, dt)
    far = T.worst(ref["exact"]["grad"], ref["rounded"]["grad"], ref["rounded"]["grad_bound"])
    print(f"max |exact - rounded| / bound on grad_kqv = {far:.2f}")
    assert far >= 2.0, far
