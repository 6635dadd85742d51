"""The opt-in 16-bit matrix inputs of the attention layer without a GPU: the `attention=` flag of `ptgnn_amd.precision`,
the shape predicate and the C ABI of csrc/block_attention16.hip as far as they go without a device, and the layer's CPU
route (`torch_route.self_attention_message_passing(inputs=)`) against the float64 restatement of
tests/attention_inputs_cases.py with the normalised probabilities rounded."""
import ctypes
import os
import re

import pytest
import torch

import attention_inputs_cases as A
import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ptgnn_amd_attention16_block", "ptgnn_amd_attention16_block_supported"]
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
EINVAL, EUNSUPPORTED = -1, -2


class OnGpu:              # what `resolve` reads of a tensor
    is_cuda = True


def _state():
    """(dtype setting, edge_gemm, training, mlp, attention): the flags as their `*_inputs` functions show them."""
    import ptgnn_amd
    from ptgnn_amd import precision
    v = ptgnn_amd.get_matrix_inputs()
    on = v in C.HALF
    return (v, on and precision.edge_gemm_inputs(OnGpu()) is v, on and precision.training_inputs(OnGpu()) is v,
            on and precision.mlp_inputs(OnGpu()) is v, on and precision.attention_inputs(OnGpu()) is v)


OFF = (torch.float32, False, False, False, False)


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_off_and_calls_without_the_keyword_leave_it_off():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.attention_inputs is precision.attention_inputs
    cpu = torch.zeros(1)
    assert _state() == OFF and precision.attention_inputs(cpu) is torch.float32
    for v in C.HALF:
        for kw in ({}, {"edge_gemm": True}, {"training": True}, {"mlp": True},
                   {"edge_gemm": True, "training": True, "mlp": True}):
            with ptgnn_amd.matrix_inputs(v, **kw):                       # every existing call: attention stays fp32
                assert _state() == (v, kw.get("edge_gemm", False), kw.get("training", False), kw.get("mlp", False), False)
                assert precision.attention_inputs(cpu) is torch.float32 and precision.resolve(cpu) is v
            assert ptgnn_amd.set_matrix_inputs(v, **kw) is torch.float32
            assert _state()[4] is False
            assert ptgnn_amd.set_matrix_inputs(torch.float32) is v
    assert _state() == OFF


def test_keyword_sets_the_flag_independently_and_float32_resets_everything():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu = torch.zeros(1)
    for v in C.HALF:
        assert ptgnn_amd.set_matrix_inputs(v, attention=True) is torch.float32     # still the previous DTYPE setting
        assert _state() == (v, False, False, False, True) and precision.attention_inputs(cpu) is v
        assert ptgnn_amd.set_matrix_inputs(v) is v                                 # without the keyword: flag off again
        assert _state() == (v, False, False, False, False)
        ptgnn_amd.set_matrix_inputs(v, edge_gemm=True, training=True, mlp=True, attention=True)
        assert _state() == (v, True, True, True, True)
        assert ptgnn_amd.set_matrix_inputs(torch.float32) is v                     # resets all five
        assert _state() == OFF
        ptgnn_amd.set_matrix_inputs(v)
        assert _state() == (v, False, False, False, False)                         # ... so the flag did not survive
        ptgnn_amd.set_matrix_inputs(torch.float32)
    assert ptgnn_amd.set_matrix_inputs(torch.float32, attention=True) is torch.float32   # accepted, and means fp32
    assert precision.attention_inputs(cpu) is torch.float32 and precision.attention_inputs(OnGpu()) is torch.float32
    ptgnn_amd.set_matrix_inputs(torch.float32)
    with pytest.raises(TypeError):
        ptgnn_amd.set_matrix_inputs(torch.bfloat16, False, False, False, True)     # keyword only
    assert _state() == OFF


def test_context_manager_restores_all_five_values_also_after_an_exception():
    import ptgnn_amd
    bf, hf = C.HALF
    ptgnn_amd.set_matrix_inputs(hf, edge_gemm=True, mlp=True)
    try:
        with ptgnn_amd.matrix_inputs(bf, attention=True):
            assert _state() == (bf, False, False, False, True)
            with ptgnn_amd.matrix_inputs(hf, training=True, attention=True):
                assert _state() == (hf, False, True, False, True)
            assert _state() == (bf, False, False, False, True)
        assert _state() == (hf, True, False, True, False)
        with pytest.raises(RuntimeError, match="boom"):
            with ptgnn_amd.matrix_inputs(bf, attention=True):
                raise RuntimeError("boom")
        assert _state() == (hf, True, False, True, False)
        ptgnn_amd.set_matrix_inputs(bf, training=True, attention=True)
        with pytest.raises(RuntimeError, match="boom"):
            with ptgnn_amd.matrix_inputs(hf):
                assert _state() == (hf, False, False, False, False)
                raise RuntimeError("boom")
        assert _state() == (bf, False, True, False, True)
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    assert _state() == OFF


def test_attention_inputs_resolves_autocast_like_resolve():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu = torch.zeros(1)
    prev = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        for flag in (False, True):
            with ptgnn_amd.matrix_inputs("autocast", attention=flag):
                torch.set_autocast_enabled("cuda", False)
                assert precision.attention_inputs(OnGpu()) is torch.float32               # no autocast region
                torch.set_autocast_enabled("cuda", True)
                for dt in C.HALF + (torch.float32,):
                    torch.set_autocast_dtype("cuda", dt)
                    assert precision.attention_inputs(OnGpu()) is (dt if flag else torch.float32)
                    assert precision.attention_inputs(cpu) is torch.float32               # never touches CPU tensors
    finally:
        torch.set_autocast_enabled("cuda", prev[0])
        torch.set_autocast_dtype("cuda", prev[1])
    assert _state() == OFF


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_signatures_and_launch_family_of_the_16_bit_attention():
    from ptgnn_amd import _lib, build as B, ops
    assert "block_attention16.hip" in B.SOURCES and "block_attention.hip" in B.SOURCES
    path = B.build()
    text = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    assert "selfattmessagepassing.py:104-117" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(ptgnn_amd_attention16[a-z0-9_]*)\s*\(", code))) == SYMBOLS
    raw = ctypes.CDLL(path)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "attention16" in s) == SYMBOLS
    lib = _lib.load()
    assert lib.ptgnn_amd_version() == 102                          # additive entries: the ABI version stays
    # a family range of its own, after the existing ones; the earlier ranges end where they did
    assert lib.ptgnn_amd_launch_name(768) == b"block_attention16" and lib.ptgnn_amd_launch_name(769) is None
    assert lib.ptgnn_amd_launch_name(706) is None and lib.ptgnn_amd_launch_name(75) == b"block_attention"
    assert lib.ptgnn_amd_launch_count(768) >= 0 and lib.ptgnn_amd_launch_count(769) == -1
    assert "block_attention16" not in ops.launch_counts(aggregation=True, half=True, half_training=True)
    assert "block_attention16" in ops.launch_counts(attention16=True)
    before = ops.launch_counts(attention16=True)
    assert ops.launches_since(before) == {}


def test_supported_over_the_width_grid_and_a_bad_dtype_id():
    from ptgnn_amd import _lib, ops
    lib = _lib.load()
    for dt_id, dt in ((BF16, torch.bfloat16), (F16, torch.float16)):
        for dk in (0, 1, 8, 17, 32, 127, 128, 129):
            for dv in (0, 1, 6, 48, 128, 129):
                want = 1 <= dk <= 128 and 1 <= dv <= 128
                assert lib.ptgnn_amd_attention16_block_supported(dk, dv, dt_id) == int(want), (dk, dv)
                assert lib.ptgnn_amd_block_attention_supported(dk, dv) == int(want)       # the widths of the fp32 kernel
                assert ops.block_attention16_supported(dk, dv, dt) is want
    for bad in (0, 3, -1):
        assert lib.ptgnn_amd_attention16_block_supported(32, 32, bad) == 0
    assert ops.block_attention16_supported(32, 32, torch.float32) is False
    assert ops.block_attention16_supported(32, 32, torch.float64) is False


def test_entry_refuses_bad_arguments_before_any_device_call():
    from ptgnn_amd import _lib
    lib = _lib.load()

    def call(dk=32, dv=32, dtype=BF16, ld=96, ld_out=32, rows=10, windows=3, max_nodes=40, heads=1):
        return lib.ptgnn_amd_attention16_block(None, ld, None, windows, rows, max_nodes, heads, dk, dv, None, ld_out, None,
                                               dtype, None)
    assert call(dtype=3) == EINVAL and b"dtype" in lib.ptgnn_amd_last_error()
    assert call() == EINVAL and b"block_attention16" in lib.ptgnn_amd_last_error()        # null pointers
    assert call(dk=129) == EUNSUPPORTED and b"block_attention16" in lib.ptgnn_amd_last_error()
    assert call(max_nodes=0) == EINVAL and call(heads=0) == EINVAL
    assert call(rows=0) == 0                                                              # nothing to do


def test_ops_keyword_is_checked_and_cpu_tensors_are_refused():
    import inspect
    from ptgnn_amd import PtgnnAmdError, ops
    assert inspect.signature(ops.block_attention).parameters["inputs"].default is None
    assert inspect.signature(ops.launch_counts).parameters["attention16"].default is False
    with pytest.raises(PtgnnAmdError):
        ops.block_attention(torch.randn(4, 12), torch.zeros(2, dtype=torch.int32), 4, 1, 4, 4, inputs=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
@pytest.mark.parametrize("dk,dv", [(32, 32), (17, 6), (8, 8)], ids=["k32v32", "k17v6", "k8v8"])
def test_cpu_block_attention_is_inside_the_bound_with_two_roundings(dt, dk, dv):
    """torch_route.block_attention(inputs=dt) against `rounded` with the NORMALISED probabilities rounded too: the bound
    of the GPU test with 2 u in place of u (P / l is rounded after the normalisation: one rounding more), and the
    exact-fp32 route far outside it."""
    from ptgnn_amd import torch_route
    heads = 3
    c = A.case("max33", heads, dk, dv, dt)
    kqv, windows = c["kqv"], c["windows"]
    with torch.no_grad():
        got = torch_route.block_attention(kqv, windows, heads, dk, dv, inputs=dt).double()
        plain = torch_route.block_attention(kqv, windows, heads, dk, dv).double()
    rounded, _, weight, length = A.attention64(kqv, windows, heads, dk, dv, dt)
    vmax = float(A.rnd(kqv.reshape(kqv.shape[0], heads, -1)[..., 2 * dk:], dt).abs().max())
    bound = A.out_bound(rounded, weight, length, vmax, dt, roundings=2)
    ratio = (got - rounded).abs() / bound
    print(f"max |got - rounded| / bound = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0
    assert float(((plain - rounded).abs() / bound).max()) >= 2.0          # the flag did something


def _cpu_layer(p=0.0):
    from ptgnn_amd import layers as L
    torch.manual_seed(8300)
    layer = L.MultiHeadSelfAttentionMessagePassing(64, 16, 16, 64, 128, 2, dropout_rate=p, max_num_nodes=33)
    counts = [40, 33, 5]
    x = torch.randn(sum(counts), 64, generator=torch.Generator().manual_seed(8301))
    idx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    return layer, x, idx


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_layer_rounds_under_the_flag_and_keeps_its_bits_everywhere_else(dt):
    import inspect
    import ptgnn_amd
    from ptgnn_amd import torch_route
    assert inspect.signature(torch_route.self_attention_message_passing).parameters["inputs"].default is torch.float32
    layer, x, idx = _cpu_layer()
    layer.eval()
    with torch.no_grad():
        default = layer(x, [], idx, {}, {}, [])
        with ptgnn_amd.matrix_inputs(dt, attention=True):
            got = layer(x, [], idx, {}, {}, [])
            again = layer(x, [], idx, {}, {}, [])
        assert torch.equal(got, again) and not torch.equal(got, default) and bool(torch.isfinite(got).all())
        # the same operands rounded by hand
        want = torch_route.self_attention_message_passing(
            x, x, idx, *(getattr(layer, "_MultiHeadSelfAttentionMessagePassing__" + n) for n in (
                "selfatt_head_transforms", "summarization_layer", "intermediate_layer", "output_layer", "layer_norm1",
                "layer_norm2", "dropout_layer")), 2, 16, 16, 33, inputs=dt)
        assert torch.equal(got, want)
        for args, kw in (((dt,), {}), ((dt,), dict(edge_gemm=True, training=True, mlp=True)),
                         ((torch.float32,), dict(attention=True)), (("autocast",), dict(attention=True))):
            with ptgnn_amd.matrix_inputs(*args, **kw):
                assert torch.equal(layer(x, [], idx, {}, {}, []), default), (args, kw)


@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_layer_that_needs_a_gradient_keeps_the_default_bits_under_the_flag(dt):
    import ptgnn_amd
    layer, x, idx = _cpu_layer()
    layer.train()                                                           # dropout 0: train() only asks for gradients

    def step():
        layer.zero_grad()
        y = layer(x, [], idx, {}, {}, [])
        y.square().sum().backward()
        return y.detach().clone(), [p.grad.clone() for p in layer.parameters()]

    y0, g0 = step()
    with ptgnn_amd.matrix_inputs(dt, attention=True):
        y1, g1 = step()
    assert torch.equal(y1, y0) and all(torch.equal(u, v) for u, v in zip(g1, g0))
