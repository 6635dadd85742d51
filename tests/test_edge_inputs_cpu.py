"""The opt-in 16-bit matrix inputs of the grouped per-edge GEMM without a GPU: the `edge_gemm=` flag of
`ptgnn_amd.precision`, the C ABI of csrc/edge_gemm16.hip as far as it goes without a device (symbols, launch counters,
the shape predicate, every argument check from fake pointers), and the GGNN layer's CPU route, which already rounds the
message operands under the dtype setting and which the flag must not change."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = sorted(["ptgnn_amd_edge_linear16_supported", "ptgnn_amd_edge_linear16", "ptgnn_amd_edge_linear16_shared"])
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def _state():
    """(dtype setting, whether the per-edge GEMM follows it) -- the flag is observable through edge_gemm_inputs alone."""
    import ptgnn_amd
    from ptgnn_amd import precision
    v = ptgnn_amd.get_matrix_inputs()
    probe = torch.zeros(1)
    return v, v in C.HALF and precision.edge_gemm_inputs(probe) is v


def test_flag_defaults_off_and_calls_without_the_keyword_leave_it_off():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.edge_gemm_inputs is precision.edge_gemm_inputs
    cpu = torch.zeros(1)
    assert _state() == (torch.float32, False) and precision.edge_gemm_inputs(cpu) is torch.float32
    for v in C.HALF:
        with ptgnn_amd.matrix_inputs(v):                               # today's call: the per-edge GEMM stays fp32
            assert _state() == (v, False) and precision.edge_gemm_inputs(cpu) is torch.float32
            assert precision.resolve(cpu) is v
        assert ptgnn_amd.set_matrix_inputs(v) is torch.float32
        assert _state() == (v, False)
        assert ptgnn_amd.set_matrix_inputs(torch.float32) is v
    assert _state() == (torch.float32, False)


def test_keyword_sets_the_flag_and_float32_resets_everything():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu = torch.zeros(1)
    for v in C.HALF:
        assert ptgnn_amd.set_matrix_inputs(v, edge_gemm=True) is torch.float32       # still the previous DTYPE setting
        assert _state() == (v, True) and precision.edge_gemm_inputs(cpu) is v
        assert ptgnn_amd.set_matrix_inputs(v) is v                                   # without the keyword: flag off again
        assert _state() == (v, False)
        ptgnn_amd.set_matrix_inputs(v, edge_gemm=True)
        assert ptgnn_amd.set_matrix_inputs(torch.float32) is v                       # resets both
        assert _state() == (torch.float32, False)
        ptgnn_amd.set_matrix_inputs(v)
        assert _state() == (v, False)                                                # ... so the flag did not survive
        ptgnn_amd.set_matrix_inputs(torch.float32)
    # edge_gemm=True with float32 is accepted and means fp32
    assert ptgnn_amd.set_matrix_inputs(torch.float32, edge_gemm=True) is torch.float32
    assert precision.edge_gemm_inputs(cpu) is torch.float32 and precision.resolve(cpu) is torch.float32
    ptgnn_amd.set_matrix_inputs(torch.float32)
    with pytest.raises(TypeError):
        ptgnn_amd.set_matrix_inputs(torch.bfloat16, True)                            # keyword only
    assert _state() == (torch.float32, False)


def test_contexts_restore_both_values_nested_and_after_an_exception():
    import ptgnn_amd
    bf, fp = torch.bfloat16, torch.float16
    with ptgnn_amd.matrix_inputs(bf, edge_gemm=True):
        assert _state() == (bf, True)
        with ptgnn_amd.matrix_inputs(fp):                      # an inner existing-style call turns the flag off ...
            assert _state() == (fp, False)
            with ptgnn_amd.matrix_inputs(fp, edge_gemm=True):
                assert _state() == (fp, True)
            assert _state() == (fp, False)
        assert _state() == (bf, True)                          # ... and leaving it turns the flag back on
        with pytest.raises(ZeroDivisionError):
            with ptgnn_amd.matrix_inputs(torch.float32):
                assert _state() == (torch.float32, False)
                1 / 0
        assert _state() == (bf, True)
    assert _state() == (torch.float32, False)
    with pytest.raises(ZeroDivisionError):
        with ptgnn_amd.matrix_inputs(bf, edge_gemm=True):
            1 / 0
    assert _state() == (torch.float32, False)
    ptgnn_amd.set_matrix_inputs(bf)                            # a context inside a plain set: back to exactly that
    try:
        with ptgnn_amd.matrix_inputs(fp, edge_gemm=True):
            assert _state() == (fp, True)
        assert _state() == (bf, False)
    finally:
        ptgnn_amd.set_matrix_inputs(torch.float32)
    for bad in (torch.float64, "bf16", None):                  # a bad value leaves both alone
        with ptgnn_amd.matrix_inputs(bf, edge_gemm=True):
            with pytest.raises(ptgnn_amd.PtgnnAmdError):
                ptgnn_amd.set_matrix_inputs(bad, edge_gemm=False)
            assert _state() == (bf, True)
    assert _state() == (torch.float32, False)


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


def test_edge_gemm_inputs_resolves_autocast_like_resolve():
    import ptgnn_amd
    from ptgnn_amd import precision

    class OnGpu:            # what `resolve` reads of a tensor
        is_cuda = True
    cpu = torch.zeros(1)
    for flag in (False, True):
        with ptgnn_amd.matrix_inputs("autocast", edge_gemm=flag):
            assert precision.edge_gemm_inputs(OnGpu()) is torch.float32                       # no autocast region
            for dt in C.HALF + (torch.float32,):
                with _gpu_autocast_state(True, dt):
                    assert precision.edge_gemm_inputs(OnGpu()) is (dt if flag else torch.float32)
                    assert precision.edge_gemm_inputs(cpu) is torch.float32                   # never touches CPU tensors
                with _gpu_autocast_state(False, dt):
                    assert precision.edge_gemm_inputs(OnGpu()) is torch.float32
    assert _state() == (torch.float32, False)


# ---------------------------------------------------------------------------------------------------------------------
# the GGNN layer on CPU tensors: the route already rounds the message operands; the flag changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_cpu_layer_gives_the_same_bits_with_and_without_the_flag(dt):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(8300)
    layer = L.GatedMessagePassingLayer(64, 64, 8, "sum").eval()
    x = torch.randn(90, 64, generator=torch.Generator().manual_seed(8301))
    adj = C.random_adjacency(90, (25,) * 8, 8302)                 # the edge-form proportions of the GPU tests
    feats = [torch.empty(a[0].shape[0], 0) for a in adj]
    with torch.no_grad():
        default = layer(x, adj, None, {}, {}, feats)
        with ptgnn_amd.matrix_inputs(dt):
            off = layer(x, adj, None, {}, {}, feats)
        with ptgnn_amd.matrix_inputs(dt, edge_gemm=True):
            on = layer(x, adj, None, {}, {}, feats)
        with ptgnn_amd.matrix_inputs(torch.float32, edge_gemm=True):
            fp32_on = layer(x, adj, None, {}, {}, feats)
    assert torch.equal(on, off) and not torch.equal(off, default)
    assert torch.equal(fp32_on, default)
    with ptgnn_amd.matrix_inputs(dt, edge_gemm=True):
        out = layer(x, adj, None, {}, {}, feats)                  # grad mode on: a training call ignores both
    assert out.requires_grad and torch.equal(out.detach(), default)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_exports_ctypes_and_library_agree_on_the_three_symbols(lib):
    from ptgnn_amd import _lib, build as B
    assert "edge_gemm16.hip" in B.SOURCES and lib.ptgnn_amd_version() == 102       # additive: the ABI version stays
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_edge_linear16[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    exports = open(os.path.join(ROOT, "ptgnn_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ptgnn_amd_\*;", exports) and re.search(r"local:\s*\*;", exports)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(s for s in _lib.SIGNATURES if "edge_linear16" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    pinned = ("_half_", "beam", "decode_step", "embedding_bag", "graph_norm", "segment_scores", "vocab_loss",
              "copy_loss_finish", "logit_loss", "candidate_scores", "char_embed", "_window_", "block_attention",
              "attention_windows")
    assert not [s for s in SYMBOLS if any(p in s for p in pinned)]
    assert lib.ptgnn_amd_half_supported(2, 64, 64, BF16) == 0            # the half kinds did not grow a third


def test_edge16_counters_have_their_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_launch_name(512) == b"edge16" and lib.ptgnn_amd_launch_name(513) == b"edge16_shared"
    assert lib.ptgnn_amd_launch_name(514) is None and lib.ptgnn_amd_launch_name(511) is None
    assert lib.ptgnn_amd_launch_count(512) >= 0 and lib.ptgnn_amd_launch_count(513) >= 0
    assert lib.ptgnn_amd_launch_count(514) == -1
    for first, count in ((0, 13), (64, 17), (128, 4), (192, 4), (256, 3), (320, 1), (384, 1), (448, 2), (512, 2)):
        assert lib.ptgnn_amd_launch_name(first + count - 1) is not None, first
        assert lib.ptgnn_amd_launch_name(first + count) is None, first
    default = list(ops.launch_counts())
    assert list(ops.launch_counts(edge16=True)) == default + ["edge16", "edge16_shared"]
    assert list(ops.launch_counts(half=True, edge16=True)) == default + ["half_linear", "half_gru", "edge16",
                                                                        "edge16_shared"]
    everything_else = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True,
                                        beam=True, half=True)
    assert "edge16" not in everything_else and "edge16_shared" not in everything_else
    before = ops.launch_counts(edge16=True)
    assert ops.launches_since(before) == {}                              # launches_since reads the new range too
    before["edge16_shared"] -= 1
    assert ops.launches_since(before) == {"edge16_shared": 1}


def test_supported_predicate_over_the_shape_grid(lib):
    from ptgnn_amd import ops
    sup = lib.ptgnn_amd_edge_linear16_supported
    for dt in (BF16, F16):
        for h in (32, 64, 96, 128, 256, 1024):
            for m in (32, 64, 160, 1024):
                for t in (2, 8, 17, 64):
                    assert sup(h, m, t, dt) == 1, (h, m, t)
        for h, m, t in ((64, 36, 8), (48, 64, 8), (64, 64, 1), (64, 64, 65), (64, 64, 0), (64, 64, -3), (0, 64, 8),
                        (64, 0, 8), (-32, 64, 8), (16, 64, 8), (1056, 64, 8), (64, 1056, 8), (64, 30, 8), (36, 36, 8)):
            assert sup(h, m, t, dt) == 0, (h, m, t)
    for dt in (0, 3, -1):
        assert sup(64, 64, 8, dt) == 0
    assert ops.edge_linear16_supported(128, 128, 17, torch.bfloat16)
    assert ops.edge_linear16_supported(64, 160, 2, torch.float16)
    assert not ops.edge_linear16_supported(64, 36, 8, torch.bfloat16)
    assert not ops.edge_linear16_supported(64, 64, 1, torch.float16)
    assert not ops.edge_linear16_supported(64, 64, 8, torch.float32)


def test_entries_refuse_bad_arguments_before_anything_touches_the_device(lib):
    """The pointers are fake and never dereferenced (the per-type arrays are real HOST arrays, as the ABI says): every
    call below must answer from the argument checks."""
    p = 0x1000                      # 16-byte aligned, never dereferenced
    T = 3
    Ptr, Cnt = ctypes.c_void_p * T, ctypes.c_int64 * T

    def per_edge(counts=(5, 0, 40), srcs=(p, None, p), h=64, m=64, t=T, act=0, dt=BF16, x=p, w=p, msg=p, ld_x=64,
                 ld_msg=64, num_rows=10, src_array=True, count_array=True):
        sp = ctypes.cast(Ptr(*srcs), ctypes.c_void_p) if src_array else None
        cn = ctypes.cast(Cnt(*counts), ctypes.c_void_p) if count_array else None
        return lib.ptgnn_amd_edge_linear16(x, ld_x, num_rows, h, sp, cn, w, t, m, act, dt, msg, ld_msg, None)

    def shared(h=64, m=64, t=T, act=0, dt=BF16, x=p, w=p, msg=p, table=p, ld_x=64, ld_msg=64, num_rows=10):
        return lib.ptgnn_amd_edge_linear16_shared(x, ld_x, num_rows, h, table, w, t, m, act, dt, msg, ld_msg, None)

    def message():
        return lib.ptgnn_amd_last_error().decode()

    def refused(rc, code, *words):
        msg = message()
        return rc == code and msg.startswith("edge_linear16:") and all(w in msg for w in words)

    # no rows: no launch, no error -- whatever the operand pointers are
    assert per_edge(counts=(0, 0, 0), srcs=(None, None, None)) == 0
    assert per_edge(counts=(0, 0, 0), srcs=(None, None, None), x=None, w=None, msg=None, src_array=False) == 0
    for entry in (per_edge, shared):
        for dt in (0, 3):
            assert refused(entry(dt=dt), EINVAL, "dtype")
        assert refused(entry(act=3), EINVAL, "act") and refused(entry(act=-1), EINVAL, "act")
        assert refused(entry(h=0), EINVAL, "sizes") and refused(entry(m=-64), EINVAL, "sizes")
        assert refused(entry(t=0), EINVAL, "sizes")
        assert refused(entry(m=36), EUNSUPPORTED, "msg_dim=36")
        assert refused(entry(h=48, ld_x=48), EUNSUPPORTED, "state_dim=48")
        assert refused(entry(h=1056, ld_x=1056), EUNSUPPORTED) and refused(entry(m=1056, ld_msg=1056), EUNSUPPORTED)
        assert refused(entry(t=1), EUNSUPPORTED, "num_types=1")
        assert refused(entry(x=None), EINVAL, "null") and refused(entry(w=None), EINVAL, "null")
        assert refused(entry(msg=None), EINVAL, "null")
        assert refused(entry(num_rows=0), EINVAL) and refused(entry(num_rows=-1), EINVAL)
        assert refused(entry(ld_x=32), EINVAL) and refused(entry(ld_msg=32), EINVAL)
        # operands the loads cannot read
        assert refused(entry(x=p + 4), EUNSUPPORTED, "aligned") and refused(entry(ld_x=66), EUNSUPPORTED, "aligned")
        assert refused(entry(w=p + 2), EUNSUPPORTED, "aligned") and refused(entry(msg=p + 2), EUNSUPPORTED, "aligned")
    assert refused(shared(t=65), EUNSUPPORTED, "num_types=65")
    assert refused(shared(table=None), EINVAL, "table")
    assert refused(shared(num_rows=1 << 31), EUNSUPPORTED, "too many")               # beyond the table's int32 keys
    assert refused(per_edge(count_array=False), EINVAL, "counts")
    assert refused(per_edge(counts=(5, -1, 40)), EINVAL, "negative")
    assert refused(per_edge(srcs=(p, None, None)), EINVAL, "type 2")
    assert refused(per_edge(src_array=False), EINVAL, "type 0")
    assert refused(per_edge(counts=(5, 0, 1 << 36)), EUNSUPPORTED, "too many")       # beyond the int32 unit range
    assert refused(per_edge(counts=(0, 0, 0), m=36), EUNSUPPORTED)                    # the shape is checked before the rows


def test_ops_keywords_refuse_what_the_16_bit_form_does_not_take():
    """Raised before anything touches a tensor: the forms with dropout, edge features or a target-state half are fp32."""
    from ptgnn_amd import _lib, ops
    x = torch.zeros(4, 32)
    adj = [(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))] * 2
    ws = [torch.zeros(32, 32)] * 2
    for kwargs in ({"use_dst": True}, {"use_dst": False, "dropout": (1, 0.5, 7)},
                   {"use_dst": False, "edge_feats": [torch.zeros(3, 4)] * 2}):
        with pytest.raises(_lib.PtgnnAmdError, match="16-bit inputs"):
            ops.edge_linear(x, adj, ws, inputs=torch.bfloat16, **kwargs)
    with pytest.raises(_lib.PtgnnAmdError, match="inputs must be"):
        ops.edge_linear(x, adj, ws, False, inputs="autocast")
