"""The opt-in 16-bit matrix inputs of the MLP-MP layer without a GPU: the `mlp=` flag of `ptgnn_amd.precision`, the
layer's CPU route (`torch_route.mlp_layer(inputs=)`) against the float64 restatement of tests/mlp_half_cases.py, the
preconditions of the GPU tests' layer cases, and the C ABI of the per-edge GEMM with a target-state half as far as it goes
without a device (symbols, launch counter, the shape predicate, argument checks from fake pointers)."""
import ctypes
import os
import re

import pytest
import torch

import half_cases as C
import mlp_half_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ptgnn_amd_edge_dst_linear16", "ptgnn_amd_edge_dst_linear16_supported"]
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def _state():
    """(dtype setting, edge_gemm, training, mlp) -- the flags are observable through their `*_inputs` functions."""
    import ptgnn_amd
    from ptgnn_amd import precision

    class OnGpu:            # what `resolve` / `training_inputs` read of a tensor
        is_cuda = True
    v = ptgnn_amd.get_matrix_inputs()
    on = v in C.HALF
    return (v, on and precision.edge_gemm_inputs(OnGpu()) is v, on and precision.training_inputs(OnGpu()) is v,
            on and precision.mlp_inputs(OnGpu()) is v)


def test_flag_defaults_off_and_calls_without_the_keyword_leave_it_off():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.mlp_inputs is precision.mlp_inputs
    cpu = torch.zeros(1)
    assert _state() == (torch.float32, False, False, False) and precision.mlp_inputs(cpu) is torch.float32
    for v in C.HALF:
        for kw in ({}, {"edge_gemm": True}, {"training": True}, {"edge_gemm": True, "training": True}):
            with ptgnn_amd.matrix_inputs(v, **kw):                         # every existing call: MLP-MP stays fp32
                assert _state() == (v, kw.get("edge_gemm", False), kw.get("training", False), False)
                assert precision.mlp_inputs(cpu) is torch.float32 and precision.resolve(cpu) is v
            assert ptgnn_amd.set_matrix_inputs(v, **kw) is torch.float32
            assert _state()[3] is False
            assert ptgnn_amd.set_matrix_inputs(torch.float32) is v
    assert _state() == (torch.float32, False, False, False)


def test_keyword_sets_the_flag_and_float32_resets_everything():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu = torch.zeros(1)
    for v in C.HALF:
        assert ptgnn_amd.set_matrix_inputs(v, mlp=True) is torch.float32             # still the previous DTYPE setting
        assert _state() == (v, False, False, True) and precision.mlp_inputs(cpu) is v
        assert ptgnn_amd.set_matrix_inputs(v) is v                                   # without the keyword: flag off again
        assert _state() == (v, False, False, False)
        ptgnn_amd.set_matrix_inputs(v, edge_gemm=True, training=True, mlp=True)
        assert _state() == (v, True, True, True)
        assert ptgnn_amd.set_matrix_inputs(torch.float32) is v                       # resets all four
        assert _state() == (torch.float32, False, False, False)
        ptgnn_amd.set_matrix_inputs(v)
        assert _state() == (v, False, False, False)                                  # ... so the flag did not survive
        ptgnn_amd.set_matrix_inputs(torch.float32)
    assert ptgnn_amd.set_matrix_inputs(torch.float32, mlp=True) is torch.float32     # accepted, and means fp32
    assert precision.mlp_inputs(cpu) is torch.float32 and precision.resolve(cpu) is torch.float32
    ptgnn_amd.set_matrix_inputs(torch.float32)
    with pytest.raises(TypeError):
        ptgnn_amd.set_matrix_inputs(torch.bfloat16, False, False, True)              # keyword only
    assert _state() == (torch.float32, False, False, False)


def test_contexts_restore_all_four_values_nested_and_after_an_exception():
    import ptgnn_amd
    bf, fp = torch.bfloat16, torch.float16
    with ptgnn_amd.matrix_inputs(bf, edge_gemm=True, mlp=True):
        assert _state() == (bf, True, False, True)
        with ptgnn_amd.matrix_inputs(fp, training=True):           # an inner existing-style call turns the flag off ...
            assert _state() == (fp, False, True, False)
            with ptgnn_amd.matrix_inputs(fp, mlp=True):
                assert _state() == (fp, False, False, True)
            assert _state() == (fp, False, True, False)
        assert _state() == (bf, True, False, True)                 # ... and leaving it turns the flag back on
        with pytest.raises(ZeroDivisionError):
            with ptgnn_amd.matrix_inputs(torch.float32):
                assert _state() == (torch.float32, False, False, False)
                1 / 0
        assert _state() == (bf, True, False, True)
    assert _state() == (torch.float32, False, False, False)
    ptgnn_amd.set_matrix_inputs(bf, training=True)                 # a context inside a plain set: back to exactly that
    try:
        with ptgnn_amd.matrix_inputs(fp, mlp=True):
            assert _state() == (fp, False, False, True)
        assert _state() == (bf, False, True, False)
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    for bad in (torch.float64, "bf16", None):                      # a bad value leaves all four alone
        with ptgnn_amd.matrix_inputs(bf, mlp=True):
            with pytest.raises(ptgnn_amd.PtgnnAmdError):
                ptgnn_amd.set_matrix_inputs(bad, mlp=False)
            assert _state() == (bf, False, False, True)
    assert _state() == (torch.float32, False, False, False)


def test_mlp_inputs_resolves_autocast_like_resolve():
    import ptgnn_amd
    from ptgnn_amd import precision

    class OnGpu:
        is_cuda = True
    cpu = torch.zeros(1)
    prev = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        for flag in (False, True):
            with ptgnn_amd.matrix_inputs("autocast", mlp=flag):
                torch.set_autocast_enabled("cuda", False)
                assert precision.mlp_inputs(OnGpu()) is torch.float32                     # no autocast region
                torch.set_autocast_enabled("cuda", True)
                for dt in C.HALF + (torch.float32,):
                    torch.set_autocast_dtype("cuda", dt)
                    assert precision.mlp_inputs(OnGpu()) is (dt if flag else torch.float32)
                    assert precision.mlp_inputs(cpu) is torch.float32                     # never touches CPU tensors
    finally:
        torch.set_autocast_enabled("cuda", prev[0])
        torch.set_autocast_dtype("cuda", prev[1])
    assert _state() == (torch.float32, False, False, False)


# ---------------------------------------------------------------------------------------------------------------------
# the layer on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(MC.LAYER_SEEDS), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{'dst' if k[3] else 'src'}")
def test_cpu_layer_matches_float64_on_the_rounded_operands_and_the_gpu_cases_hold_their_preconditions(key):
    """Every layer case of tests/test_gpu_mlp_inputs.py, on the CPU route: the exact-fp32 route is inside the bar of
    float64 (the case's LayerNorm amplifies nothing beyond it), rounding moves the result by >= 20 bars, and under
    `mlp=True` the route is within the bar of the rounded reference."""
    import ptgnn_amd
    layer, x, adj = MC.layer_case(*key, MC.LAYER_SEEDS[key])
    weights = layer.export_weights()
    exact = MC.mlp64(x, adj, weights)
    with torch.no_grad():
        default = MC.run_layer(layer, x, adj)
        assert C.err(default, exact) <= C.bar(exact)
        for dt in C.HALF:
            with ptgnn_amd.matrix_inputs(dt, mlp=True):
                got = MC.run_layer(layer, x, adj)
            MC.check(got, MC.mlp64(x, adj, weights, dt=dt), exact, f"CPU layer {key} {C.IDS[dt]}")
            with ptgnn_amd.matrix_inputs(dt, edge_gemm=True, training=True):            # without the flag: today's bits
                assert torch.equal(MC.run_layer(layer, x, adj), default)
            with ptgnn_amd.matrix_inputs("autocast", mlp=True):
                assert torch.equal(MC.run_layer(layer, x, adj), default)                # "autocast": never on CPU tensors
        with ptgnn_amd.matrix_inputs(torch.float32, mlp=True):
            assert torch.equal(MC.run_layer(layer, x, adj), default)


@pytest.mark.parametrize("form", ["edge", "table"])
def test_cpu_pna_layer_matches_float64_on_the_rounded_operands(form):
    import ptgnn_amd
    layer, x, adj = MC.layer_case(form, 64, "pna", True, MC.PNA_SEEDS[form], pna=True)
    weights = layer.export_weights()
    exact = MC.mlp64(x, adj, weights, pna_delta=1.5)
    with torch.no_grad():
        assert C.err(MC.run_layer(layer, x, adj), exact) <= C.bar(exact)
        for dt in C.HALF:
            with ptgnn_amd.matrix_inputs(dt, mlp=True):
                got = MC.run_layer(layer, x, adj)
            MC.check(got, MC.mlp64(x, adj, weights, dt=dt, pna_delta=1.5), exact, f"CPU PNA layer {form} {C.IDS[dt]}")


def test_torch_route_keyword_and_what_stays_fp32_on_the_cpu():
    import inspect
    import ptgnn_amd
    from ptgnn_amd import layers as L, torch_route
    assert inspect.signature(torch_route.mlp_layer).parameters["inputs"].default is torch.float32
    n = MC.N_NODES
    g = torch.Generator().manual_seed(8700)
    torch.manual_seed(8701)
    x, adj = torch.randn(n, 64, generator=g), MC.adjacency(n, MC.UNIT_ROWS, 8704)
    feats = [torch.randn(int(s.shape[0]), 8, generator=g) for s, _ in adj]
    dt = torch.bfloat16

    class SubclassedPna(L.PnaMessageAggregation):      # the routes round under exactly PnaMessageAggregation
        pass
    for layer, f in ((L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum", mlp_hidden_layers=1).eval(), None),
                     (L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum", features_dimension=8).eval(), feats),
                     (L.MlpMessagePassingLayer(64, 64, 64, len(adj), SubclassedPna(delta=1.5)).eval(), None)):
        with torch.no_grad():
            default = MC.run_layer(layer, x, adj, f)
            with ptgnn_amd.matrix_inputs(dt, mlp=True):
                assert torch.equal(MC.run_layer(layer, x, adj, f), default)
    layer = L.MlpMessagePassingLayer(64, 64, 64, len(adj), "sum").eval()
    with torch.no_grad():
        default = MC.run_layer(layer, x, adj)
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            assert not torch.equal(MC.run_layer(layer, x, adj), default)
    with ptgnn_amd.matrix_inputs(dt, mlp=True):
        out = MC.run_layer(layer, x, adj)                             # grad mode on: a training call stays fp32
    assert out.requires_grad and torch.equal(out.detach(), default)
    # a GGNN layer under `mlp=True` alone is the GGNN layer under the plain dtype setting
    ggnn = L.GatedMessagePassingLayer(64, 64, len(adj), "sum").eval()
    with torch.no_grad():
        with ptgnn_amd.matrix_inputs(dt):
            plain = MC.run_layer(ggnn, x, adj)
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            assert torch.equal(MC.run_layer(ggnn, x, adj), plain)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_library_and_host_agree_on_the_two_symbols(lib):
    from ptgnn_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(ptgnn_amd_edge_dst_[a-z0-9_]*)\s*\(", text))) == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    assert "mlpmessagepassing.py:88-98" in header and hasattr(ops, "edge_linear16_dst_supported")


def test_counter_has_its_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_launch_name(640) == b"edge16_dst" and lib.ptgnn_amd_launch_name(641) is None
    assert lib.ptgnn_amd_launch_name(639) is None
    assert lib.ptgnn_amd_launch_count(640) >= 0 and lib.ptgnn_amd_launch_count(641) == -1
    default = list(ops.launch_counts())
    assert list(ops.launch_counts(edge16_dst=True)) == default + ["edge16_dst"]
    assert list(ops.launch_counts(edge16=True, edge16_dst=True)) == default + ["edge16", "edge16_shared", "edge16_dst"]
    before = ops.launch_counts(edge16_dst=True)
    assert ops.launches_since(before) == {}                              # launches_since reads the new range too
    before["edge16_dst"] -= 1
    assert ops.launches_since(before) == {"edge16_dst": 1}


def test_supported_predicate_over_the_shape_grid(lib):
    from ptgnn_amd import ops
    sup = lib.ptgnn_amd_edge_dst_linear16_supported
    for dt in (BF16, F16):
        for h in (32, 64, 96, 128, 256, 1024):
            for m in (32, 64, 128, 160, 1024):
                for t in (2, 8, 21, 64):
                    assert sup(h, m, t, dt) == 1, (h, m, t)
        for h, m, t in ((64, 36, 8), (48, 64, 8), (64, 64, 1), (64, 64, 65), (64, 64, 0), (64, 64, -3), (0, 64, 8),
                        (64, 0, 8), (-32, 64, 8), (16, 64, 8), (1056, 64, 8), (64, 1056, 8), (64, 30, 8), (36, 36, 8)):
            assert sup(h, m, t, dt) == 0, (h, m, t)
    for dt in (0, 3, -1):
        assert sup(64, 64, 8, dt) == 0
    assert ops.edge_linear16_dst_supported(64, 64, 21, torch.bfloat16)
    assert ops.edge_linear16_dst_supported(256, 160, 2, torch.float16)
    assert not ops.edge_linear16_dst_supported(64, 36, 8, torch.bfloat16)
    assert not ops.edge_linear16_dst_supported(64, 64, 1, torch.float16)
    assert not ops.edge_linear16_dst_supported(64, 64, 8, torch.float32)


def test_entry_refuses_bad_arguments_before_anything_touches_the_device(lib):
    """The pointers are fake and never dereferenced (the per-type arrays are real HOST arrays, as the ABI says): every
    call below must answer from the argument checks."""
    p = 0x1000                      # 16-byte aligned, never dereferenced
    T = 3
    Ptr, Cnt = ctypes.c_void_p * T, ctypes.c_int64 * T

    def entry(counts=(5, 0, 40), srcs=(p, None, p), dsts=(p, None, p), h=64, m=64, t=T, act=0, dt=BF16, x=p, w=p, msg=p,
              ld_x=64, ld_msg=64, num_rows=10, src_array=True, dst_array=True, count_array=True):
        sp = ctypes.cast(Ptr(*srcs), ctypes.c_void_p) if src_array else None
        dp = ctypes.cast(Ptr(*dsts), ctypes.c_void_p) if dst_array else None
        cn = ctypes.cast(Cnt(*counts), ctypes.c_void_p) if count_array else None
        return lib.ptgnn_amd_edge_dst_linear16(x, ld_x, num_rows, h, sp, dp, cn, w, t, m, act, dt, msg, ld_msg, None)

    def refused(rc, code, *words):
        msg = lib.ptgnn_amd_last_error().decode()
        return rc == code and msg.startswith("edge_linear16: dst:") and all(w in msg for w in words)

    # no rows: no launch, no error -- whatever the operand pointers are
    assert entry(counts=(0, 0, 0), srcs=(None,) * 3, dsts=(None,) * 3) == 0
    assert entry(counts=(0, 0, 0), srcs=(None,) * 3, x=None, w=None, msg=None, src_array=False, dst_array=False) == 0
    for dt in (0, 3):
        assert refused(entry(dt=dt), EINVAL, "dtype")
    assert refused(entry(act=3), EINVAL, "act") and refused(entry(act=-1), EINVAL, "act")
    assert refused(entry(h=0), EINVAL, "sizes") and refused(entry(m=-64), EINVAL, "sizes")
    assert refused(entry(t=0), EINVAL, "sizes")
    assert refused(entry(m=36), EUNSUPPORTED, "msg_dim=36")
    assert refused(entry(h=48, ld_x=48), EUNSUPPORTED, "state_dim=48")
    assert refused(entry(h=1056, ld_x=1056), EUNSUPPORTED) and refused(entry(m=1056, ld_msg=1056), EUNSUPPORTED)
    assert refused(entry(t=1), EUNSUPPORTED, "num_types=1") and refused(entry(t=65), EUNSUPPORTED, "num_types=65")
    assert refused(entry(x=None), EINVAL, "null") and refused(entry(w=None), EINVAL, "null")
    assert refused(entry(msg=None), EINVAL, "null")
    assert refused(entry(num_rows=0), EINVAL) and refused(entry(num_rows=-1), EINVAL)
    assert refused(entry(ld_x=32), EINVAL) and refused(entry(ld_msg=32), EINVAL)
    assert refused(entry(x=p + 4), EUNSUPPORTED, "aligned") and refused(entry(ld_x=66), EUNSUPPORTED, "aligned")
    assert refused(entry(w=p + 2), EUNSUPPORTED, "aligned") and refused(entry(msg=p + 2), EUNSUPPORTED, "aligned")
    assert refused(entry(count_array=False), EINVAL, "counts")
    assert refused(entry(counts=(5, -1, 40)), EINVAL, "negative")
    assert refused(entry(srcs=(p, None, None)), EINVAL, "source ids", "type 2")
    assert refused(entry(dsts=(p, None, None)), EINVAL, "target ids", "type 2")
    assert refused(entry(src_array=False), EINVAL, "type 0") and refused(entry(dst_array=False), EINVAL, "target ids")
    assert refused(entry(counts=(5, 0, 1 << 36)), EUNSUPPORTED, "too many")          # beyond the int32 unit range
    assert refused(entry(counts=(0, 0, 0), m=36), EUNSUPPORTED)                       # the shape is checked before the rows


def test_ops_keywords_on_cpu_tensors():
    """Raised before anything touches a tensor's data."""
    from ptgnn_amd import _lib, ops
    x = torch.zeros(4, 32)
    adj = [(torch.zeros(3, dtype=torch.int64), torch.ones(3, dtype=torch.int64))] * 2
    ws = [torch.zeros(32, 64)] * 2
    with pytest.raises(_lib.PtgnnAmdError, match="16-bit inputs with a target-state half"):
        ops.edge_linear(x, adj, ws, True, inputs=torch.bfloat16)
    with pytest.raises(_lib.PtgnnAmdError, match="neither dropout nor edge features"):
        ops.edge_linear(x, adj, ws, True, inputs=torch.float16, edge_feats=[torch.zeros(3, 4)] * 2)
    with pytest.raises(_lib.PtgnnAmdError, match="inputs must be"):
        ops.edge_linear(x, adj, ws, True, inputs="autocast")
