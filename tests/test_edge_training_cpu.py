"""The opt-in 16-bit matrix inputs of the GGNN edge-form training step without a GPU: the `edge_training=` flag of
`ptgnn_amd.precision`, the C ABI of the masked forms of csrc/edge_gemm16.hip and of csrc/edge_wgrad16.hip as far as it
goes without a device (symbols, launch counters, the shape predicates, the chunk and workspace queries, the argument
checks from fake pointers), the layer's CPU training route (which the flag must not change), and the precondition of
every random case of tests/test_gpu_edge_training.py: on each, the float64 references on the exact and on the rounded
operands are at least 20 bars apart under an arbitrary Bernoulli mask, and under the hash mask the GPU tests run with
(restated on the CPU)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import edge_training_cases as E
import half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = sorted(["ptgnn_amd_edge_masked_linear16", "ptgnn_amd_edge_masked_linear16_supported",
                  "ptgnn_amd_edge_weight_grad16", "ptgnn_amd_edge_weight_grad16_supported",
                  "ptgnn_amd_edge_wgrad16_chunk_edges", "ptgnn_amd_edge_wgrad16_workspace_bytes"])
BF16, F16 = 1, 2          # PTGNN_AMD_HALF_BF16 / _F16
EINVAL, EUNSUPPORTED = -1, -2
FLAGS = ("edge_gemm", "training", "mlp", "attention", "edge_training")


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
def _flags():
    from ptgnn_amd import precision
    return tuple(getattr(precision, "_" + f) for f in FLAGS)


def test_flag_defaults_off_is_scoped_and_float32_resets_it():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert ptgnn_amd.edge_training_inputs is precision.edge_training_inputs
    for fn in (ptgnn_amd.set_matrix_inputs, ptgnn_amd.matrix_inputs):
        params = inspect.signature(fn).parameters
        assert list(params)[1:] == list(FLAGS), list(params)                 # the fifth keyword, after the other four
        assert params["edge_training"].default is False and params["edge_training"].kind is inspect.Parameter.KEYWORD_ONLY
    assert ptgnn_amd.get_matrix_inputs() is torch.float32 and _flags() == (False,) * 5
    for v in C.HALF:
        with ptgnn_amd.matrix_inputs(v):                                     # today's call: the flag stays off
            assert _flags() == (False,) * 5
        with ptgnn_amd.matrix_inputs(v, edge_training=True):
            assert ptgnn_amd.get_matrix_inputs() is v and _flags() == (False, False, False, False, True)
            with ptgnn_amd.matrix_inputs(v, training=True):                  # every call without the keyword: off
                assert _flags() == (False, True, False, False, False)
            assert _flags() == (False, False, False, False, True)
        assert ptgnn_amd.get_matrix_inputs() is torch.float32 and _flags() == (False,) * 5
        assert ptgnn_amd.set_matrix_inputs(v, edge_training=True) is torch.float32
        assert _flags()[4] is True
        assert ptgnn_amd.set_matrix_inputs(v) is v and _flags()[4] is False
        ptgnn_amd.set_matrix_inputs(v, edge_training=True)
        assert ptgnn_amd.set_matrix_inputs(torch.float32) is v               # resets it
        assert _flags() == (False,) * 5
    with pytest.raises(ptgnn_amd.PtgnnAmdError):
        ptgnn_amd.set_matrix_inputs(torch.float64, edge_training=True)
    assert _flags() == (False,) * 5


def test_flag_is_independent_of_the_other_four():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu = torch.zeros(1)
    readers = {"edge_gemm": precision.edge_gemm_inputs, "mlp": precision.mlp_inputs,
               "attention": precision.attention_inputs}
    for v in C.HALF:
        with ptgnn_amd.matrix_inputs(v, edge_training=True):                 # alone: the others read fp32
            assert all(r(cpu) is torch.float32 for r in readers.values())
            assert precision.training_inputs(cpu) is torch.float32 and precision.resolve(cpu) is v
        for other in FLAGS[:4]:
            with ptgnn_amd.matrix_inputs(v, **{other: True}):                # any other alone: this one off
                assert _flags() == tuple(f == other for f in FLAGS)
            with ptgnn_amd.matrix_inputs(v, **{other: True}, edge_training=True):
                assert _flags() == tuple(f in (other, "edge_training") for f in FLAGS)
        with ptgnn_amd.matrix_inputs(v, edge_gemm=True, training=True):      # pinned by existing tests: unchanged
            assert _flags() == (True, True, False, False, False)


def test_edge_training_inputs_is_float32_on_cpu_tensors_and_without_the_flag():
    import ptgnn_amd
    from ptgnn_amd import precision
    cpu, meta = torch.zeros(1), torch.zeros(1, device="meta")
    assert precision.edge_training_inputs(cpu) is torch.float32
    for v in C.HALF:
        with ptgnn_amd.matrix_inputs(v, edge_training=True):
            assert precision.edge_training_inputs(cpu) is torch.float32      # CPU tensors: fp32 in training
            assert precision.edge_training_inputs(meta) is torch.float32     # (is_cuda decides, as training_inputs)
        with ptgnn_amd.matrix_inputs(v, training=True, edge_gemm=True, mlp=True, attention=True):
            assert precision.edge_training_inputs(cpu) is torch.float32
    with ptgnn_amd.matrix_inputs(torch.float32, edge_training=True):         # accepted, means fp32
        assert precision._edge_training is True and precision.edge_training_inputs(cpu) is torch.float32
    with ptgnn_amd.matrix_inputs("autocast", edge_training=True):
        assert precision.edge_training_inputs(cpu) is torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_exports_ctypes_and_library_agree_on_the_new_entries(lib):
    from ptgnn_amd import _lib, build as B, ops
    assert "edge_wgrad16.hip" in B.SOURCES and lib.ptgnn_amd_version() == 102       # additive: the ABI version stays
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_edge_(?:masked_linear16|weight_grad16|wgrad16)[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    exports = open(os.path.join(ROOT, "ptgnn_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ptgnn_amd_\*;", exports) and re.search(r"local:\s*\*;", exports)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
        args = re.search(r"\b" + s + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[s][1]) == len(args.split(",")), s     # one ctypes entry per declared parameter
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))
    assert "gatedmessagepassing.py:57-61" in header and 'edge_linear16: masked:' in header
    for name in ("edge_linear16_masked_supported", "edge_weight_grad16_supported", "edge_wgrad16_chunk_edges"):
        assert hasattr(ops, name), name
    assert inspect.signature(ops.edge_weight_grad).parameters["inputs"].default is None
    from ptgnn_amd import scatter
    assert inspect.signature(scatter.edge_linear).parameters["inputs"].default is None


def test_training_launches_have_their_own_range_and_keyword(lib):
    from ptgnn_amd import ops
    names = [b"edge16_masked", b"edge_wgrad16"]
    assert [lib.ptgnn_amd_launch_name(832 + i) for i in range(3)] == names + [None]
    assert lib.ptgnn_amd_launch_name(831) is None and lib.ptgnn_amd_launch_count(834) == -1
    assert all(lib.ptgnn_amd_launch_count(832 + i) >= 0 for i in range(2))
    for first, count in ((512, 2), (576, 3), (640, 1), (704, 2), (768, 1)):      # the earlier ranges end where they ended
        assert lib.ptgnn_amd_launch_name(first + count) is None and lib.ptgnn_amd_launch_name(first + count - 1) is not None
    params = list(inspect.signature(ops.launch_counts).parameters)
    assert params[-1] == "edge16_training" and inspect.signature(ops.launch_counts).parameters["edge16_training"].default is False
    default = list(ops.launch_counts())
    assert list(ops.launch_counts(edge16_training=True)) == default + [n.decode() for n in names]
    everything_else = ops.launch_counts(aggregation=True, char_cnn=True, heads=True, sequence=True, decode=True, beam=True,
                                        half=True, edge16=True, half_training=True, edge16_dst=True, beam_finish=True,
                                        attention16=True)
    assert not [n for n in E.MASKED_FAMILIES if n in everything_else]
    before = ops.launch_counts(edge16_training=True)
    assert ops.launches_since(before) == {}                              # launches_since reads the new range too
    before["edge_wgrad16"] -= 1
    assert ops.launches_since(before) == {"edge_wgrad16": 1}


def test_supported_predicates_over_the_shape_grid(lib):
    from ptgnn_amd import ops
    masked, wgrad = lib.ptgnn_amd_edge_masked_linear16_supported, lib.ptgnn_amd_edge_weight_grad16_supported
    plain = lib.ptgnn_amd_edge_linear16_supported
    good = [(h, m, t) for h in (32, 64, 96, 128, 256, 1024) for m in (32, 64, 160, 1024) for t in (2, 8, 17, 64)]
    bad = [(64, 36, 8), (48, 64, 8), (64, 64, 1), (64, 64, 65), (64, 64, 0), (64, 64, -3), (0, 64, 8), (64, 0, 8),
           (-32, 64, 8), (16, 64, 8), (1056, 64, 8), (64, 1056, 8), (64, 30, 8), (36, 36, 8)]
    for dt in (BF16, F16):
        for h, m, t in good:
            assert wgrad(h, m, t, dt) == 1 and masked(h, m, t, dt, 1) == 1 and masked(h, m, t, dt, 2) == 1, (h, m, t)
            for mode in (0, 3, -1):                                      # the masked form is mode 1 or 2
                assert masked(h, m, t, dt, mode) == 0
        for h, m, t in bad:
            assert wgrad(h, m, t, dt) == 0 and masked(h, m, t, dt, 1) == 0 and masked(h, m, t, dt, 2) == 0, (h, m, t)
            assert plain(h, m, t, dt) == 0                               # the remaining limits are edge_linear16's
    for dt in (0, 3, -1):
        assert wgrad(64, 64, 8, dt) == 0 and masked(64, 64, 8, dt, 1) == 0
    assert ops.edge_linear16_masked_supported(128, 128, 17, torch.bfloat16, 1)
    assert ops.edge_linear16_masked_supported(96, 160, 5, torch.float16, 2)
    assert not ops.edge_linear16_masked_supported(48, 64, 5, torch.bfloat16, 1)
    assert not ops.edge_linear16_masked_supported(64, 64, 5, torch.bfloat16, 0)
    assert not ops.edge_linear16_masked_supported(64, 64, 5, torch.float32, 1)
    assert ops.edge_weight_grad16_supported(128, 128, 17, torch.bfloat16)
    assert not ops.edge_weight_grad16_supported(128, 128, 1, torch.float16)
    assert not ops.edge_weight_grad16_supported(128, 100, 17, torch.float16)
    assert not ops.edge_weight_grad16_supported(128, 128, 17, torch.float32)


def test_chunk_and_workspace_queries(lib):
    from ptgnn_amd import ops
    chunk, bytes_ = lib.ptgnn_amd_edge_wgrad16_chunk_edges, lib.ptgnn_amd_edge_wgrad16_workspace_bytes
    for h, m in E.WGRAD_SHAPES + E.EDGE_SHAPES:
        for edges in (0, 1, 600, 512 * 3):
            assert chunk(edges, 4, m, h) == E.MIN_CHUNK, (h, m, edges)     # the floor, at every test size
        counts = E.wgrad_counts(E.MIN_CHUNK)
        assert ops.edge_wgrad16_chunk_edges(sum(counts), len(counts), m, h) == E.MIN_CHUNK
        assert bytes_(0, 4, m, h) == 0
        total = sum(counts)
        chunks = sum(-(-c // E.MIN_CHUNK) for c in counts)
        assert bytes_(total, 4, m, h) >= chunks * m * h * 4               # room for one partial per chunk
        assert bytes_(total, 4, m, h) == (total // E.MIN_CHUNK + 4) * m * h * 4
    big = chunk(625_000, 17, 128, 128)                                    # the Graph2Class layer: about 512 workgroups
    assert big % 32 == 0 and big > E.MIN_CHUNK and 400 <= 625_000 // big <= 512
    assert chunk(625_000, 17, 128, 256) == 2 * big or abs(chunk(625_000, 17, 128, 256) - 2 * big) <= 32   # two tiles
    for h, m, t in ((48, 64, 4), (64, 36, 4), (64, 64, 1), (64, 64, 65), (2048, 64, 4)):
        assert chunk(600, t, m, h) == 0 and bytes_(600, t, m, h) == 0
    assert chunk(-1, 4, 64, 64) == 0


def test_entries_refuse_bad_arguments_before_anything_touches_the_device(lib):
    """The pointers are fake and never dereferenced (the per-type arrays are real HOST arrays, as the ABI says): every
    call below must answer from the argument checks."""
    p = 0x1000                      # 16-byte aligned, never dereferenced
    T = 3
    Ptr, Cnt = ctypes.c_void_p * T, ctypes.c_int64 * T

    def message():
        return lib.ptgnn_amd_last_error().decode()

    def masked(counts=(5, 0, 40), srcs=(p, None, p), h=64, m=64, t=T, dt=BF16, x=p, w=p, msg=p, ld_x=64, ld_msg=64,
               num_rows=10, mode=1, prob=0.25, bits=p, src_array=True, count_array=True):
        sp = ctypes.cast(Ptr(*srcs), ctypes.c_void_p) if src_array else None
        cn = ctypes.cast(Cnt(*counts), ctypes.c_void_p) if count_array else None
        return lib.ptgnn_amd_edge_masked_linear16(x, ld_x, num_rows, h, sp, cn, w, t, m, dt, msg, ld_msg, mode, prob,
                                                  bits, None)

    def refused(rc, code, *words):
        msg = message()
        return rc == code and msg.startswith("edge_linear16: masked:") and all(w in msg for w in words)

    assert masked(counts=(0, 0, 0), srcs=(None, None, None)) == 0          # no rows: no launch, no error
    assert masked(counts=(0, 0, 0), srcs=(None, None, None), x=None, w=None, msg=None, bits=None, src_array=False) == 0
    for dt in (0, 3):
        assert refused(masked(dt=dt), EINVAL, "dtype")
    for mode in (-1, 3):
        assert refused(masked(mode=mode), EINVAL, "dropout")
    assert refused(masked(prob=1.0), EINVAL, "dropout") and refused(masked(prob=-0.1), EINVAL, "dropout")
    assert refused(masked(h=0), EINVAL, "sizes") and refused(masked(m=-64), EINVAL, "sizes")
    assert refused(masked(t=0), EINVAL, "sizes")
    assert refused(masked(m=36), EUNSUPPORTED, "msg_dim=36")
    assert refused(masked(h=48, ld_x=48), EUNSUPPORTED, "state_dim=48")
    assert refused(masked(t=1), EUNSUPPORTED, "num_types=1") and refused(masked(t=65), EUNSUPPORTED, "num_types=65")
    assert refused(masked(x=None), EINVAL, "null") and refused(masked(w=None), EINVAL, "null")
    assert refused(masked(msg=None), EINVAL, "null")
    assert refused(masked(num_rows=0), EINVAL) and refused(masked(ld_x=32), EINVAL) and refused(masked(ld_msg=32), EINVAL)
    assert refused(masked(x=p + 4), EUNSUPPORTED, "aligned") and refused(masked(w=p + 2), EUNSUPPORTED, "aligned")
    assert refused(masked(msg=p + 2), EUNSUPPORTED, "aligned") and refused(masked(bits=p + 2), EUNSUPPORTED, "mask_bits")
    assert refused(masked(count_array=False), EINVAL, "counts")
    assert refused(masked(counts=(5, -1, 40)), EINVAL, "negative")
    assert refused(masked(srcs=(p, None, None)), EINVAL, "type 2")
    assert refused(masked(counts=(5, 0, 1 << 36)), EUNSUPPORTED, "too many")

    def wgrad(counts=(5, 0, 40), srcs=(p, None, p), h=64, m=64, t=T, dt=BF16, x=p, g=p, gw=p, ws=p, ws_bytes=1 << 30,
              ld_x=64, ld_g=64, num_rows=10, prob=0.25, bits=p, src_array=True, count_array=True):
        sp = ctypes.cast(Ptr(*srcs), ctypes.c_void_p) if src_array else None
        cn = ctypes.cast(Cnt(*counts), ctypes.c_void_p) if count_array else None
        return lib.ptgnn_amd_edge_weight_grad16(x, ld_x, num_rows, h, sp, cn, g, ld_g, t, m, dt, prob, bits, gw, ws,
                                                ws_bytes, None)

    def refused_w(rc, code, *words):
        msg = message()
        return rc == code and msg.startswith("edge_weight_grad16:") and all(w in msg for w in words)

    for dt in (0, 3):
        assert refused_w(wgrad(dt=dt), EINVAL, "dtype")
    assert refused_w(wgrad(prob=1.0), EINVAL, "dropout") and refused_w(wgrad(prob=-0.5), EINVAL, "dropout")
    assert refused_w(wgrad(h=0), EINVAL, "sizes") and refused_w(wgrad(t=0), EINVAL, "sizes")
    assert refused_w(wgrad(m=36), EUNSUPPORTED, "msg_dim=36") and refused_w(wgrad(h=48, ld_x=48), EUNSUPPORTED, "state_dim=48")
    assert refused_w(wgrad(t=1), EUNSUPPORTED, "num_types=1") and refused_w(wgrad(t=65), EUNSUPPORTED, "num_types=65")
    assert refused_w(wgrad(gw=None), EINVAL, "null") and refused_w(wgrad(count_array=False), EINVAL, "null")
    assert refused_w(wgrad(gw=p + 4), EUNSUPPORTED, "aligned")
    assert refused_w(wgrad(counts=(5, -1, 40)), EINVAL, "negative")
    assert refused_w(wgrad(x=None), EINVAL, "null") and refused_w(wgrad(g=None), EINVAL, "null")
    assert refused_w(wgrad(src_array=False), EINVAL, "null")
    assert refused_w(wgrad(num_rows=0), EINVAL) and refused_w(wgrad(ld_x=32), EINVAL) and refused_w(wgrad(ld_g=32), EINVAL)
    assert refused_w(wgrad(num_rows=1 << 31), EUNSUPPORTED, "too many rows")
    assert refused_w(wgrad(x=p + 4), EUNSUPPORTED, "aligned") and refused_w(wgrad(ld_g=66), EUNSUPPORTED, "aligned")
    assert refused_w(wgrad(bits=p + 2), EUNSUPPORTED, "mask_bits")
    assert refused_w(wgrad(srcs=(p, None, None)), EINVAL, "type 2")
    assert refused_w(wgrad(ws_bytes=16), EINVAL, "workspace") and refused_w(wgrad(ws=None), EINVAL, "workspace")
    assert refused_w(wgrad(ws=p + 8), EINVAL, "workspace")


def test_ops_keywords_on_cpu_tensors():
    """Raised before anything touches a tensor's data: dropout comes to the 16-bit form as bits, without a target half."""
    from ptgnn_amd import _lib, ops
    x = torch.zeros(4, 32)
    adj = [(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))] * 2
    ws = [torch.zeros(32, 32)] * 2
    with pytest.raises(_lib.PtgnnAmdError, match="16-bit inputs take dropout only as mask_bits"):
        ops.edge_linear(x, adj, ws, False, inputs=torch.bfloat16, dropout=(1, 0.5, 7))
    bits = torch.zeros(6, 1, dtype=torch.int32)
    with pytest.raises(_lib.PtgnnAmdError, match="16-bit inputs take dropout only as mask_bits"):
        ops.edge_linear(x, adj, ws, True, inputs=torch.float16, dropout=(1, 0.5, 7), mask_bits=bits)
    with pytest.raises(_lib.PtgnnAmdError, match="neither dropout nor edge features"):
        ops.edge_linear(x, adj, ws, False, inputs=torch.float16, edge_feats=[torch.zeros(3, 4)] * 2)


# ---------------------------------------------------------------------------------------------------------------------
# the layer's CPU route: training under the flag is bit-equal to no flag
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_step(layer, x, adj):
    torch.manual_seed(9001)
    layer.zero_grad()
    x = x.detach().clone().requires_grad_(True)
    feats = [torch.empty(int(s.shape[0]), 0) for s, _ in adj]
    out = layer(x, adj, None, {}, {}, feats)
    out.backward(torch.ones_like(out))
    return [out.detach()] + [p.grad.clone() for p in layer.parameters()] + [x.grad.clone()]


@pytest.mark.parametrize("dropout", [0.0, 0.2])
def test_cpu_training_under_the_flag_is_bit_equal_to_no_flag(dropout):
    import ptgnn_amd
    from ptgnn_amd import layers as L
    torch.manual_seed(9000)
    layer = L.GatedMessagePassingLayer(64, 64, 3, "sum", dropout_rate=dropout)
    layer.train()
    x = torch.randn(40, 64, generator=torch.Generator().manual_seed(9002))
    adj = C.random_adjacency(40, (30, 0, 17), 9003)
    plain = _cpu_step(layer, x, adj)
    for v in C.HALF + ("autocast", torch.float32):
        with ptgnn_amd.matrix_inputs(v, edge_training=True):
            flagged = _cpu_step(layer, x, adj)
        assert len(flagged) == len(plain) and all(torch.equal(a, b) for a, b in zip(flagged, plain)), v
        with ptgnn_amd.matrix_inputs(v, edge_training=True, training=True):
            flagged = _cpu_step(layer, x, adj)
        assert all(torch.equal(a, b) for a, b in zip(flagged, plain)), v


# ---------------------------------------------------------------------------------------------------------------------
# the GPU tests' random cases tell the two float64 references apart (the precondition of their check())
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", C.HALF, ids=C.IDS.get)
def test_every_random_case_separates_the_references_under_a_bernoulli_mask(dt):
    for h, m in E.EDGE_SHAPES:
        x, ws, adj, g = E.edge_case(h, m)
        for keep in (E.bernoulli_keep(g.shape[0], h, E.P, 9300 + h + m), E.hash_keep(g.shape[0], h, E.P, E.SEED)):
            for what, (rounded, exact, bar) in E.references(x, ws, adj, g, keep, E.P, dt).items():
                gap = C.err(exact, rounded)
                print(f"  {C.IDS[dt]} ({h}, {m}) {what}: bar {bar:.3e} gap {gap:.3e} = {gap / bar:.0f} bars")
                assert gap >= C.MARGIN * bar, (h, m, what, gap, bar)
    for h, m in E.WGRAD_SHAPES:                     # (the GPU tests without a mask compare bits, not float64)
        x, ws, adj, g = E.wgrad_case(h, m)
        for keep in (E.bernoulli_keep(g.shape[0], h, E.P, 9400 + h + m), E.hash_keep(g.shape[0], h, E.P, E.SEED), None):
            rounded, exact, bar = E.references(x, ws, adj, g, keep, E.P, dt)["d_w"]
            gap = C.err(exact, rounded)
            print(f"  {C.IDS[dt]} ({h}, {m}) d_w {'masked' if keep is not None else 'plain'}: bar {bar:.3e} gap {gap:.3e}")
            assert gap >= C.MARGIN * bar, (h, m, gap, bar)
            assert not bool(rounded[1].any())                              # the empty type's row is zeros
