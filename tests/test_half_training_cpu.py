"""The opt-in 16-bit matrix inputs of the GGNN training step without a GPU: the `training=` keyword of the
`ptgnn_amd.precision` switch, the new C-ABI entries as far as they go without a device (csrc/wgrad16.hip and the
training forms in csrc/half_gemm.hip), and the CPU layer, which stays fp32 in training under every setting."""
import ctypes
import os
import re

import pytest
import torch

import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = sorted(["ptgnn_amd_linear_weight_grad16", "ptgnn_amd_wgrad16_workspace_bytes", "ptgnn_amd_wgrad16_chunk_rows",
                  "ptgnn_amd_gru_cell_train16", "ptgnn_amd_linear_add16"])
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
WGRAD = 3                 # PTGNN_AMD_HALF_KIND_WGRAD
EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_training_keyword_defaults_to_false_and_float32_resets_it():
    import ptgnn_amd
    from ptgnn_amd import precision
    x = torch.zeros(2, 2)
    assert ptgnn_amd.training_inputs is precision.training_inputs
    assert precision.training_inputs(x) is torch.float32
    assert precision._training is False
    ptgnn_amd.set_matrix_inputs(torch.bfloat16)                       # without the keyword: False
    assert precision._training is False and precision.resolve(x) is torch.bfloat16
    assert ptgnn_amd.set_matrix_inputs(torch.bfloat16, training=True) is torch.bfloat16     # the previous dtype setting
    assert precision._training is True and precision._edge_gemm is False
    ptgnn_amd.set_matrix_inputs(torch.float16)                        # every call without it means False
    assert precision._training is False
    ptgnn_amd.set_matrix_inputs(torch.float16, training=True, edge_gemm=True)
    assert (precision._setting, precision._edge_gemm, precision._training) == (torch.float16, True, True)
    ptgnn_amd.set_matrix_inputs(torch.float32)                        # resets everything
    assert (precision._setting, precision._edge_gemm, precision._training) == (torch.float32, False, False)
    ptgnn_amd.set_matrix_inputs(torch.float32, training=True)         # accepted, means fp32
    assert precision.training_inputs(x) is torch.float32 and precision.resolve(x) is torch.float32
    ptgnn_amd.set_matrix_inputs(torch.float32)


def test_context_manager_restores_the_previous_triple_also_after_an_exception():
    import ptgnn_amd
    from ptgnn_amd import precision

    def triple():
        return precision._setting, precision._edge_gemm, precision._training
    assert triple() == (torch.float32, False, False)
    with ptgnn_amd.matrix_inputs(torch.bfloat16, edge_gemm=True):
        assert triple() == (torch.bfloat16, True, False)
        with ptgnn_amd.matrix_inputs(torch.float16, training=True):
            assert triple() == (torch.float16, False, True)
            with ptgnn_amd.matrix_inputs("autocast"):
                assert triple() == ("autocast", False, False)
            assert triple() == (torch.float16, False, True)
        assert triple() == (torch.bfloat16, True, False)
    assert triple() == (torch.float32, False, False)
    with pytest.raises(ZeroDivisionError):
        with ptgnn_amd.matrix_inputs(torch.bfloat16, training=True):
            1 / 0
    assert triple() == (torch.float32, False, False)
    with pytest.raises(ptgnn_amd.PtgnnAmdError):
        ptgnn_amd.set_matrix_inputs("bf16", training=True)
    assert triple() == (torch.float32, False, False)


def test_training_inputs_is_float32_for_cpu_tensors_under_every_setting(monkeypatch):
    import ptgnn_amd
    from ptgnn_amd import precision
    x = torch.zeros(2, 2)
    for v in (torch.bfloat16, torch.float16, "autocast", torch.float32):
        with ptgnn_amd.matrix_inputs(v, training=True):
            assert precision.training_inputs(x) is torch.float32, v
    # "autocast" follows torch.autocast on GPU tensors only: a CPU tensor inside a CUDA autocast region stays fp32
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    with ptgnn_amd.matrix_inputs("autocast", training=True):
        assert precision.training_inputs(x) is torch.float32 and precision.resolve(x) is torch.float32

    class OnGpu:                                     # what the layers hand over, as far as the switch looks at it
        is_cuda = True
    with ptgnn_amd.matrix_inputs("autocast", training=True):
        assert precision.training_inputs(OnGpu()) is torch.bfloat16
    with ptgnn_amd.matrix_inputs("autocast"):
        assert precision.training_inputs(OnGpu()) is torch.float32          # without the keyword
    with ptgnn_amd.matrix_inputs(torch.float16, training=True):
        assert precision.training_inputs(OnGpu()) is torch.float16


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_layer_in_training_returns_the_default_bits_under_training_true(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(7801)
    layer = L.GatedMessagePassingLayer(64, 64, 3, "sum").train()
    x = torch.randn(90, 64, generator=torch.Generator().manual_seed(7802))
    adj = C.random_adjacency(90, (120, 80, 40), 7803)
    feats = [torch.empty(a[0].shape[0], 0) for a in adj]

    def step():
        layer.zero_grad()
        out = layer(x, adj, None, {}, {}, feats)
        out.square().sum().backward()
        return out.detach().clone(), [p.grad.clone() for p in layer.parameters()]
    default, default_grads = step()
    with ptgnn_amd.matrix_inputs(dt, training=True):
        got, grads = step()
    assert torch.equal(got, default)
    assert all(torch.equal(a, b) for a, b in zip(grads, default_grads))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_library_and_host_agree_on_the_new_symbols(lib):
    from ptgnn_amd import _lib, build as B, dense, ops
    assert "wgrad16.hip" in B.SOURCES and lib.ptgnn_amd_version() == 102        # additive: the ABI version stays
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    assert "PTGNN_AMD_HALF_KIND_WGRAD = 3" in text and "gatedmessagepassing.py:57-69" in header
    for name in ("half_linear_weight_grad", "half_wgrad_chunk_rows", "HALF_KIND_WGRAD"):
        assert hasattr(ops, name), name
    assert ops.HALF_KIND_WGRAD == WGRAD
    import inspect
    for fn in (ops.gru_cell_train, ops.linear_add):
        assert {"inputs", "rounded"} <= set(inspect.signature(fn).parameters), fn
    for fn in (dense.linear, dense.gru_cell_weights, dense.gru_cell, dense._Linear.forward, dense._GruCell.forward):
        assert inspect.signature(fn).parameters["inputs"].default is None, fn


def test_training_counters_have_their_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    names = [b"half_wgrad", b"half_gru_train", b"half_linear_add"]
    assert [lib.ptgnn_amd_launch_name(576 + i) for i in range(4)] == names + [None]
    assert lib.ptgnn_amd_launch_name(575) is None and lib.ptgnn_amd_launch_count(579) == -1
    assert all(lib.ptgnn_amd_launch_count(576 + i) >= 0 for i in range(3))
    default = list(ops.launch_counts())
    assert list(ops.launch_counts(half_training=True)) == default + [n.decode() for n in names]
    assert list(ops.launch_counts(half=True)) == default + ["half_linear", "half_gru"]       # where it ended
    before = ops.launch_counts(half_training=True)
    assert ops.launches_since(before) == {}                              # launches_since reads the new range too
    before["half_wgrad"] -= 1
    assert ops.launches_since(before) == {"half_wgrad": 1}


def test_wgrad_kind_of_half_supported_at_and_around_its_limits(lib):
    from ptgnn_amd import ops
    sup = lib.ptgnn_amd_half_supported
    for dt in (BF16, F16):
        for k in (32, 64, 96, 128, 992, 1024):
            for n_out in (32, 96, 160, 384, 1024):
                assert sup(WGRAD, k, n_out, dt) == 1, (k, n_out)
        for k, n in ((30, 32), (64, 30), (0, 32), (64, 0), (-32, 32), (16, 32), (1056, 32), (32, 1056), (31, 33),
                     (1025, 32), (32, 1023)):
            assert sup(WGRAD, k, n, dt) == 0, (k, n)
        assert sup(2, 64, 64, dt) == 0 and sup(4, 64, 64, dt) == 0      # id 2 stays an unknown kind
    for dt in (0, 3, -1):
        assert sup(WGRAD, 64, 64, dt) == 0
    assert ops.half_supported(ops.HALF_KIND_WGRAD, 128, 384, torch.bfloat16)
    assert not ops.half_supported(ops.HALF_KIND_WGRAD, 128, 2048, torch.bfloat16)        # a Linear shape, not a WGRAD one
    assert ops.half_supported(ops.HALF_KIND_LINEAR, 128, 2048, torch.bfloat16)
    assert not ops.half_supported(ops.HALF_KIND_WGRAD, 64, 64, torch.float32)


def test_chunk_rows_and_workspace_need_no_device(lib):
    from ptgnn_amd import ops
    chunk, ws = lib.ptgnn_amd_wgrad16_chunk_rows, lib.ptgnn_amd_wgrad16_workspace_bytes
    for k, n_out in ((32, 32), (64, 96), (128, 384), (96, 160), (1024, 1024)):
        tiles = -(-n_out // 128) * (k // (128 if k % 128 == 0 else 64 if k % 64 == 0 else 32))
        for rows in (0, 1, 511, 512, 513, 1041, 100_000, 3_000_000):
            c = chunk(rows, n_out, k)
            assert c == ops.half_wgrad_chunk_rows(rows, n_out, k)
            assert c >= 512 and c % 32 == 0, (rows, k, n_out, c)
            parts = -(-rows // c)
            # about 512 workgroups at the most, and never a partial of fewer than 512 rows but the last
            assert parts * tiles <= 512 + tiles, (rows, k, n_out, c)
            want_rows = (rows * tiles + 511) // 512
            assert c == max(512, (want_rows + 31) // 32 * 32), (rows, k, n_out, c)
            want = 0 if parts <= 1 else parts * (n_out * k + n_out) * 4
            assert ws(rows, n_out, k) == want, (rows, k, n_out)
    assert chunk(1041, 384, 128) == 512 and chunk(513, 32, 32) == 512
    for k, n_out in ((30, 32), (32, 30), (1056, 32), (32, 1056), (0, 32)):
        assert chunk(1000, n_out, k) == 0 and ws(1000, n_out, k) == 0
    assert chunk(-1, 32, 32) == 0 and ws(-1, 32, 32) == 0


def test_new_entries_refuse_bad_arguments_before_anything_touches_the_device(lib):
    """The pointers are fake and never dereferenced; every call below must answer from the argument checks."""
    p = 0x1000                      # 16-byte aligned, never dereferenced

    def last():
        return lib.ptgnn_amd_last_error().decode()

    def wgrad(x=p, ld_x=64, k=64, g=p, ld_g=96, rows=100, n_out=96, dt=BF16, gw=p, gb=None, ws=None, ws_bytes=0):
        return lib.ptgnn_amd_linear_weight_grad16(x, ld_x, k, g, ld_g, rows, n_out, dt, gw, gb, ws, ws_bytes, None)
    assert wgrad(dt=0) == EINVAL and last().startswith("linear_weight_grad16:") and "dtype" in last()
    assert wgrad(rows=-1) == EINVAL and wgrad(k=0) == EINVAL and wgrad(gw=None) == EINVAL
    assert wgrad(k=30) == EUNSUPPORTED and "k % 32 == 0" in last()
    assert wgrad(n_out=1056, ld_g=1056) == EUNSUPPORTED and wgrad(k=1056, ld_x=1056) == EUNSUPPORTED
    assert wgrad(x=None) == EINVAL and wgrad(g=None) == EINVAL and wgrad(ld_x=32) == EINVAL and wgrad(ld_g=64) == EINVAL
    assert wgrad(x=p + 4) == EUNSUPPORTED and wgrad(ld_x=66) == EUNSUPPORTED and wgrad(ld_g=98) == EUNSUPPORTED
    assert wgrad(gw=p + 4) == EUNSUPPORTED
    assert wgrad(rows=2000) == EINVAL and "workspace" in last()         # four partials and no workspace

    def gru(a=p, ld_a=64, h=p + 0x100, ld_h=64, wi=p, wh=p, bi=p, bh=p, n=10, m=64, hd=64, dt=F16, out=p, ld_out=64,
            gates=p):
        return lib.ptgnn_amd_gru_cell_train16(a, ld_a, h, ld_h, wi, wh, bi, bh, n, m, hd, dt, out, ld_out, gates, None)
    assert gru(dt=7) == EINVAL and last().startswith("gru_cell_train16:")
    assert gru(gates=None) == EINVAL and gru(out=p + 0x100) == EINVAL and "in-place" in last()
    assert gru(m=30) == EUNSUPPORTED and gru(hd=1056, ld_h=1056, ld_out=1056) == EUNSUPPORTED
    assert gru(ld_a=66) == EUNSUPPORTED and gru(gates=p + 2) == EUNSUPPORTED
    assert gru(n=0, a=None, gates=None) == 0                            # no rows: no launch, nothing read

    def ladd(x=p, rows=10, k=64, ld_x=64, w=p, n_out=96, bias=None, act=0, dt=BF16, addend=p, ld_add=96, y=p, ld_y=96):
        return lib.ptgnn_amd_linear_add16(x, rows, k, ld_x, w, n_out, bias, act, dt, addend, ld_add, y, ld_y, None)
    assert ladd(dt=0) == EINVAL and last().startswith("linear_add16:")
    assert ladd(act=9) == EINVAL and ladd(addend=None) == EINVAL and ladd(ld_add=64) == EINVAL
    assert ladd(k=30) == EUNSUPPORTED and ladd(ld_x=66) == EUNSUPPORTED and ladd(addend=p + 2) == EUNSUPPORTED
    assert ladd(rows=0, x=None, addend=None) == 0
    # the inference entries keep their own names in their messages
    assert lib.ptgnn_amd_half_linear(p, 10, 30, 64, p, 96, None, 0, BF16, p, 96, None) == EUNSUPPORTED
    assert last().startswith("half_linear:")
