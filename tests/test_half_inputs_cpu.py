"""The opt-in 16-bit matrix inputs without a GPU: the `ptgnn_amd.precision` switch, the GGNN layer's CPU route under it
against float64 on the rounded operands (tests/half_cases.py: reference, bar and why the aggregate is taken from the
route), and the C ABI of csrc/half_gemm.hip as far as it goes without a device."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = sorted(["ptgnn_amd_half_supported", "ptgnn_amd_half_linear", "ptgnn_amd_half_gru_cell"])
DEFAULT_COUNTERS = ["k_stream_linear", "k_stream_linear_ring", "k_stream_gru", "k_stream_gru_ring", "k_stream_edge",
                    "k_stream_edge_shared", "k_stream_edge_v2", "k_wgrad_stream", "k_linear_tlp", "k_gru", "k_edge_linear",
                    "k_edge_wgrad", "k_gather_update"]
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
LINEAR, GRU = 0, 1        # PTGNN_AMD_HALF_KIND_*
EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_default_is_float32_and_the_three_functions_are_package_attributes():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.get_matrix_inputs() is torch.float32
    assert ptgnn_amd.set_matrix_inputs is precision.set_matrix_inputs
    assert ptgnn_amd.matrix_inputs is precision.matrix_inputs


def test_context_manager_restores_the_setting_also_after_an_exception():
    import ptgnn_amd
    for v in (torch.bfloat16, torch.float16, "autocast", torch.float32):
        with ptgnn_amd.matrix_inputs(v):
            assert ptgnn_amd.get_matrix_inputs() == v
            with ptgnn_amd.matrix_inputs(torch.float16):
                assert ptgnn_amd.get_matrix_inputs() is torch.float16
            assert ptgnn_amd.get_matrix_inputs() == v
        assert ptgnn_amd.get_matrix_inputs() is torch.float32
    with pytest.raises(ZeroDivisionError):
        with ptgnn_amd.matrix_inputs(torch.bfloat16):
            1 / 0
    assert ptgnn_amd.get_matrix_inputs() is torch.float32
    assert ptgnn_amd.set_matrix_inputs(torch.bfloat16) is torch.float32      # returns the previous setting
    assert ptgnn_amd.set_matrix_inputs(torch.float32) is torch.bfloat16


@pytest.mark.parametrize("bad", [torch.float64, torch.int8, "bf16", "split", 2, None])
def test_bad_values_raise_and_leave_the_setting_alone(bad):
    import ptgnn_amd
    with pytest.raises(ptgnn_amd.PtgnnAmdError):
        ptgnn_amd.set_matrix_inputs(bad)
    with pytest.raises(ptgnn_amd.PtgnnAmdError):
        with ptgnn_amd.matrix_inputs(bad):
            pass
    assert ptgnn_amd.get_matrix_inputs() is torch.float32


@contextlib.contextmanager
def _gpu_autocast_state(enabled, dtype):
    """The state `torch.autocast("cuda", dtype=...)` sets on entry -- set directly, because without a GPU the context
    manager disables itself."""
    prev = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", enabled)
    torch.set_autocast_dtype("cuda", dtype)
    try:
        yield
    finally:
        torch.set_autocast_enabled("cuda", prev[0])
        torch.set_autocast_dtype("cuda", prev[1])


def test_autocast_resolves_to_the_gpu_autocast_dtype_for_gpu_tensors_only():
    import ptgnn_amd
    from ptgnn_amd import precision

    class OnGpu:            # what `resolve` reads of a tensor
        is_cuda = True
    cpu = torch.zeros(1)
    assert precision.resolve(cpu) is torch.float32 and precision.resolve(OnGpu()) is torch.float32     # default
    with ptgnn_amd.matrix_inputs(torch.bfloat16):
        assert precision.resolve(cpu) is torch.bfloat16 and precision.resolve(OnGpu()) is torch.bfloat16
    with ptgnn_amd.matrix_inputs("autocast"):
        assert precision.resolve(OnGpu()) is torch.float32                     # no autocast region
        for dt in C.HALF + (torch.float32,):
            with _gpu_autocast_state(True, dt):
                assert precision.resolve(OnGpu()) is dt
                assert precision.resolve(cpu) is torch.float32                 # never touches CPU tensors
            with _gpu_autocast_state(False, dt):
                assert precision.resolve(OnGpu()) is torch.float32
        assert precision.resolve(OnGpu()) is torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the GGNN layer on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
N, H, T = 70, 64, 3


@pytest.fixture(scope="module")
def cpu_case():
    """reduce -> (layer, x, adjacency, edge features, default-mode output, exact float64 output): built once.
    600 edges on 70 nodes: with fewer, the fp16 rounding of a max-aggregated layer moves the float64 result by 17 - 24
    bars depending on the seed, around the 20 the precondition asks for; at this density it is 21 - 26 (fp16, max; every
    other combination is above 30).  The precondition is asserted in the test, from the two references alone."""
    from ptgnn_amd import layers as L
    out = {}
    for reduce, seed in (("sum", 8103), ("max", 8104)):
        torch.manual_seed(seed)
        layer = L.GatedMessagePassingLayer(H, H, T, reduce).eval()
        x = torch.randn(N, H, generator=torch.Generator().manual_seed(seed + 10))
        adj = C.random_adjacency(N, (300, 200, 100), seed + 20)
        feats = [torch.empty(a[0].shape[0], 0) for a in adj]
        with torch.no_grad():
            default = layer(x, adj, None, {}, {}, feats)
        exact, _ = C.ggnn64(x, adj, layer.export_weights())
        out[reduce] = (layer, x, adj, feats, default, exact)
    return out


@pytest.mark.parametrize("reduce", ["sum", "max"])
@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_layer_rounds_the_operands_the_gpu_routes_round(cpu_case, monkeypatch, reduce, dt):
    import ptgnn_amd
    from ptgnn_amd import torch_route
    layer, x, adj, feats, default, exact = cpu_case[reduce]
    weights = layer.export_weights()
    # precondition, from the references alone: rounding moves the float64 result by many bars
    rounded_f64, agg64 = C.ggnn64(x, adj, weights, linear_dt=dt, gru_dt=dt)
    bar = C.bar(rounded_f64)
    gap_f64 = C.err(exact, rounded_f64)
    print(f"  {reduce} {C.IDS[dt]}: bar {bar:.3e}, |exact - rounded| (float64 throughout) {gap_f64:.3e}")
    assert gap_f64 >= C.MARGIN * bar
    with ptgnn_amd.matrix_inputs(dt), torch.no_grad(), C.captured(monkeypatch, torch_route, "aggregate") as seen:
        got = layer(x, adj, None, {}, {}, feats)
    assert got.dtype == torch.float32 and len(seen) == 1
    # stage 1: the aggregate of the messages from rounded x and W, against float64
    e_agg = C.err(seen[0], agg64)
    print(f"    aggregate: |got - float64| {e_agg:.3e} (bar {C.bar(agg64):.3e})")
    assert e_agg <= C.bar(agg64)
    # stage 2: the GRU on the aggregate the route rounded
    want, _ = C.ggnn64(x, adj, weights, linear_dt=dt, gru_dt=dt, agg=seen[0])
    gap = C.err(exact, want)
    e, e_exact = C.err(got, want), C.err(got, exact)
    print(f"    |got - rounded| {e:.3e}, |got - exact| {e_exact:.3e}, gap {gap:.3e}")
    assert gap >= C.MARGIN * bar
    assert e <= bar
    assert e_exact >= gap - bar
    # the default setting is back and is today's route, bit for bit
    with torch.no_grad():
        assert torch.equal(layer(x, adj, None, {}, {}, feats), default)
    with ptgnn_amd.matrix_inputs(torch.float32), torch.no_grad():
        assert torch.equal(layer(x, adj, None, {}, {}, feats), default)
    assert C.err(default, exact) <= C.bar(exact)


def test_cpu_layer_ignores_the_setting_where_a_gradient_is_needed_and_under_autocast(cpu_case):
    import ptgnn_amd
    layer, x, adj, feats, default, _ = cpu_case["sum"]
    with ptgnn_amd.matrix_inputs(torch.bfloat16):
        out = layer(x, adj, None, {}, {}, feats)          # grad mode on, parameters require grad: a training call
    assert out.requires_grad and torch.equal(out.detach(), default)
    with ptgnn_amd.matrix_inputs("autocast"), _gpu_autocast_state(True, torch.bfloat16), torch.no_grad():
        assert torch.equal(layer(x, adj, None, {}, {}, feats), default)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    from ptgnn_amd import _lib, build as B
    assert "half_gemm.hip" in B.SOURCES and lib.ptgnn_amd_version() == 102
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_half_[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "_half_" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    pinned = ("beam", "decode_step", "embedding_bag", "graph_norm", "segment_scores", "vocab_loss", "copy_loss_finish",
              "logit_loss", "candidate_scores", "char_embed", "_window_", "block_attention", "attention_windows")
    assert not [s for s in SYMBOLS if any(p in s for p in pinned)]
    assert "trainer.py:205,221" in header and "abstractmessagepassing.py:43-50" in header
    assert "smallest normal" in header                                   # the small-magnitude clause of the contract


def test_half_counters_have_their_own_keyword_and_the_other_ranges_end_where_they_did(lib):
    from ptgnn_amd import ops
    assert list(ops.launch_counts()) == DEFAULT_COUNTERS
    assert list(ops.launch_counts(half=True)) == DEFAULT_COUNTERS + ["half_linear", "half_gru"]
    everything = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True, beam=True)
    assert "half_linear" not in everything and "half_gru" not in everything
    assert lib.ptgnn_amd_launch_name(448) == b"half_linear" and lib.ptgnn_amd_launch_name(449) == b"half_gru"
    assert lib.ptgnn_amd_launch_name(450) is None and lib.ptgnn_amd_launch_name(447) is None
    assert lib.ptgnn_amd_launch_count(448) >= 0 and lib.ptgnn_amd_launch_count(450) == -1
    for first, count in ((0, 13), (64, 17), (128, 4), (192, 4), (256, 3), (320, 1), (384, 1), (448, 2)):
        assert lib.ptgnn_amd_launch_name(first + count - 1) is not None, first
        assert lib.ptgnn_amd_launch_name(first + count) is None, first
    before = ops.launch_counts(half=True)
    assert ops.launches_since(before) == {}                              # launches_since reads the new range too
    before["half_gru"] -= 1
    assert ops.launches_since(before) == {"half_gru": 1}
    for mode in (2, "split"):                                            # this is not a GEMM mode
        with pytest.raises(Exception):
            ops.set_gemm_mode(mode)


def test_half_supported_is_an_argument_check(lib):
    from ptgnn_amd import ops
    sup = lib.ptgnn_amd_half_supported
    for dt in (BF16, F16):
        for k in (32, 64, 96, 128, 1024):
            for n_out in (32, 96, 160, 384, 4096):
                assert sup(LINEAR, k, n_out, dt) == 1, (k, n_out)
        for m in (32, 64, 128, 1024):
            for hd in (32, 64, 96, 128, 1024):
                assert sup(GRU, m, hd, dt) == 1, (m, hd)
        for k, n in ((30, 32), (64, 30), (0, 32), (64, 0), (-32, 32), (16, 32), (1056, 32)):
            assert sup(LINEAR, k, n, dt) == 0 and sup(GRU, k, n, dt) == 0, (k, n)
        assert sup(GRU, 64, 1056, dt) == 0 and sup(2, 64, 64, dt) == 0 and sup(-1, 64, 64, dt) == 0
    for dt in (0, 3, -1):
        assert sup(LINEAR, 64, 64, dt) == 0 and sup(GRU, 64, 64, dt) == 0
    assert ops.half_supported(ops.HALF_KIND_LINEAR, 64, 96, torch.bfloat16)
    assert ops.half_supported(ops.HALF_KIND_GRU, 64, 64, torch.float16)
    assert not ops.half_supported(ops.HALF_KIND_GRU, 64, 30, torch.bfloat16)
    assert not ops.half_supported(ops.HALF_KIND_LINEAR, 64, 64, torch.float32)
    assert (ops.HALF_IDS[torch.bfloat16], ops.HALF_IDS[torch.float16]) == (BF16, F16)
    assert (ops.HALF_KIND_LINEAR, ops.HALF_KIND_GRU) == (LINEAR, GRU)


def test_entries_refuse_bad_arguments_before_anything_touches_the_device(lib):
    """Like the int32 plan-format check of tests/test_host_cpu.py: the pointers are fake and never dereferenced; every
    call below must answer from the argument checks."""
    p = 0x1000                      # 16-byte aligned, never dereferenced

    def linear(rows=10, k=64, ld_x=64, n_out=32, act=0, dt=BF16, ld_y=32, x=p, w=p, y=p, bias=None):
        return lib.ptgnn_amd_half_linear(x, rows, k, ld_x, w, n_out, bias, act, dt, y, ld_y, None)

    def gru(n=10, m=64, hd=64, dt=BF16, ld_a=64, ld_h=64, ld_out=64, a=p, h=p, wi=p, wh=p, bi=p, bh=p, out=0x2000):
        return lib.ptgnn_amd_half_gru_cell(a, ld_a, h, ld_h, wi, wh, bi, bh, n, m, hd, dt, out, ld_out, None)

    def message():
        return lib.ptgnn_amd_last_error().decode()

    assert linear(rows=0) == 0 and gru(n=0) == 0                                     # no rows: no launch, no error
    assert linear(rows=0, x=None, w=None, y=None) == 0
    for dt in (0, 3):
        assert linear(dt=dt) == EINVAL and "dtype" in message()
        assert gru(dt=dt) == EINVAL and "dtype" in message()
    assert linear(act=3) == EINVAL and linear(rows=-1) == EINVAL and gru(n=-1) == EINVAL
    assert linear(k=30, ld_x=32) == EUNSUPPORTED and "k=30" in message()
    assert linear(n_out=30) == EUNSUPPORTED and linear(k=1056, ld_x=1056) == EUNSUPPORTED
    assert linear(rows=0, n_out=30) == EUNSUPPORTED                                  # the shape is checked before the rows
    assert gru(hd=30, ld_h=32, ld_out=32) == EUNSUPPORTED and "hd=30" in message()
    assert gru(m=48) == EUNSUPPORTED and gru(hd=1056, ld_h=1056, ld_out=1056) == EUNSUPPORTED
    assert linear(x=None) == EINVAL and linear(w=None) == EINVAL and linear(y=None) == EINVAL
    assert linear(ld_x=32) == EINVAL and linear(ld_y=16) == EINVAL
    assert gru(a=None) == EINVAL and gru(wh=None) == EINVAL and gru(bi=None) == EINVAL and gru(out=None) == EINVAL
    assert gru(ld_a=32) == EINVAL and gru(ld_out=32) == EINVAL
    assert gru(out=p) == EINVAL and "in-place" in message()
    # operands the fragment loads cannot read: rows that are not 16-byte aligned, pointers that are not float pointers
    assert linear(x=p + 4) == EUNSUPPORTED and "aligned" in message()
    assert linear(ld_x=66) == EUNSUPPORTED and linear(w=p + 2) == EUNSUPPORTED
    assert linear(y=p + 2) == EUNSUPPORTED and linear(bias=p + 1) == EUNSUPPORTED
    assert gru(a=p + 8) == EUNSUPPORTED and gru(ld_h=65) == EUNSUPPORTED and gru(wi=p + 4) == EUNSUPPORTED
    assert gru(out=0x2002) == EUNSUPPORTED and gru(bh=p + 2) == EUNSUPPORTED
    assert linear(rows=1 << 40, n_out=1 << 20, ld_y=1 << 20) == EUNSUPPORTED and "too many" in message()


def test_ops_keyword_takes_only_the_three_dtypes():
    from ptgnn_amd import _lib, ops
    assert ops._half_inputs(None) is None and ops._half_inputs(torch.float32) is None
    assert ops._half_inputs(torch.bfloat16) is torch.bfloat16 and ops._half_inputs(torch.float16) is torch.float16
    for bad in ("autocast", torch.float64, 1):
        with pytest.raises(_lib.PtgnnAmdError):
            ops._half_inputs(bad)
