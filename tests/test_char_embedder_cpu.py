"""CharUnitEmbedder on host tensors (ptgnn_amd.embeddings, the reference's operator order on torch) against fixtures of
the reference's own class (tests/golden/make_golden_charcnn.py): state_dict keys, same-seed initial parameters, the output
bit for bit and every gradient; the unfold + matmul restatement the GPU tests are judged by, pinned to the same fixtures;
plus the C ABI of csrc/char_conv.hip and of the windowed GEMM entries as far as it goes without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from char_embedder_cases import CASES, PARAMS, build, load, ref_forward, reference, state_of
from ptgnn_amd import embeddings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-5             # gradients to 2e-5 of the largest reference entry
IDS = [name for name, _ in CASES]
SPECS = dict(CASES)
SYMBOLS = ["ptgnn_amd_char_embed_backward_chunk", "ptgnn_amd_char_embed_backward_f32",
           "ptgnn_amd_char_embed_backward_workspace_bytes", "ptgnn_amd_char_embed_f32", "ptgnn_amd_char_embed_supported",
           "ptgnn_amd_window_linear_f32", "ptgnn_amd_window_max_backward_f32", "ptgnn_amd_window_max_f32",
           "ptgnn_amd_window_weight_grad_f32"]
DEFAULT_COUNTERS = ["k_stream_linear", "k_stream_linear_ring", "k_stream_gru", "k_stream_gru_ring", "k_stream_edge",
                    "k_stream_edge_shared", "k_stream_edge_v2", "k_wgrad_stream", "k_linear_tlp", "k_gru", "k_edge_linear",
                    "k_edge_wgrad", "k_gather_update"]
CHAR_COUNTERS = ["char_embed", "char_embed_backward", "window_max", "window_max_backward"]


def test_fixtures_hold_the_cases_they_are_meant_to():
    assert IDS == ["charcnn_small", "charcnn_windows_243", "charcnn_min_length", "charcnn_padded", "charcnn_odd"]
    for name, spec in CASES:
        fx = load(name)
        assert json.loads(str(fx["spec"])) == spec
        B, L, C, D = spec["B"], spec["L"], spec["C"], spec["D"]
        assert fx["chars"].shape == (B, L) and fx["chars"].dtype == np.int64
        assert fx["chars"].min() >= 0 and fx["chars"].max() < C
        assert fx["out"].shape == (B, D) and fx["coef"].shape == (B, D) and np.isfinite(fx["out"]).all()
        assert sorted(k[len("grad."):] for k in fx if k.startswith("grad.")) == sorted(PARAMS)
        assert all(np.abs(fx["grad." + k]).max() > 0 for k in PARAMS)
    small, w243, short, padded, odd = (SPECS[n] for n in IDS)
    assert (small["C"], small["L"], small["F1"], small["F2"], small["k"], small["D"], small["B"]) == \
        (40, 15, 64, 32, [3, 3, 3], 64, 9)
    assert (w243["C"], w243["L"], w243["F1"], w243["F2"], w243["k"], w243["D"], w243["B"]) == (12, 11, 8, 12, [2, 4, 3], 8, 7)
    assert short["L"] == sum(short["k"]) - 2                               # a single output position
    assert (odd["F1"], odd["F2"], odd["D"]) == (6, 12, 10)
    chars = load("charcnn_padded")["chars"]
    live = (chars != 0).sum(axis=1)
    assert set(live.tolist()) == {1, 2, 3, 4}
    assert all((row[:n] != 0).all() and not row[n:].any() for row, n in zip(chars, live))


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_state_dict_keys_and_same_seed_initial_parameters_match_the_reference(name, spec):
    want = state_of(load(name))
    torch.manual_seed(spec["seed"])
    module = build(spec, embeddings)
    assert list(module.state_dict()) == list(want) == PARAMS      # mangled names, creation order, no bias on conv_l3
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k
    build(spec, embeddings).load_state_dict(want, strict=True)
    assert [type(m).__name__ for m in module.children()] == ["Conv1d", "Conv1d", "Conv1d", "Dropout"]


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_reproduces_the_reference(name, spec):
    fx = load(name)
    module = build(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    chars, coef = torch.from_numpy(fx["chars"]), torch.from_numpy(fx["coef"])
    out = module(chars)
    assert not out.is_cuda and torch.equal(out.detach(), torch.from_numpy(fx["out"]))        # bit for bit
    (out * coef).sum().backward()
    for k, p in module.named_parameters():
        want = torch.from_numpy(fx["grad." + k])
        assert float((p.grad - want).abs().max()) <= GRAD_TOL * float(want.abs().max()), k


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_the_restatement_of_the_gpu_tests_agrees_with_the_reference_fixtures(name, spec):
    """tests/char_embedder_cases.ref_forward is the yardstick of tests/test_gpu_char_embedder.py: pinned to the reference
    here, forward and gradients, in float32 and float64."""
    fx = load(name)
    state = state_of(fx)
    params = [state[k] for k in PARAMS]
    chars, coef = torch.from_numpy(fx["chars"]), torch.from_numpy(fx["coef"])
    want = torch.from_numpy(fx["out"])
    for dtype in (torch.float32, torch.float64):
        out, grads = reference(chars, params, coef, dtype)
        assert out.dtype == dtype and ref_forward(chars, params, dtype).shape == want.shape
        assert float((out - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
        for k, g in zip(PARAMS, grads):
            w = torch.from_numpy(fx["grad." + k])
            assert float((g - w).abs().max()) <= GRAD_TOL * float(w.abs().max()), (k, dtype)


def test_exported_from_the_package():
    import ptgnn_amd
    assert ptgnn_amd.CharUnitEmbedder is embeddings.CharUnitEmbedder
    assert ptgnn_amd.CnnConfig is embeddings.CnnConfig
    assert embeddings.CnnConfig._fields == ("l1_filters", "l1_window_size", "l2_filters", "l2_window_size",
                                            "lout_window_size")


def test_host_route_is_torch_route_char_cnn():
    from ptgnn_amd import torch_route
    fx = load("charcnn_windows_243")
    module = build(SPECS["charcnn_windows_243"], embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    convs = list(module.children())[:3]
    out = torch_route.char_cnn(torch.from_numpy(fx["chars"]), SPECS["charcnn_windows_243"]["C"], *convs)
    assert torch.equal(out.detach(), torch.from_numpy(fx["out"]))


def test_cpu_tensors_never_load_the_library(monkeypatch):
    from ptgnn_amd import _lib

    def refuse():
        raise AssertionError("a CPU forward / backward loaded the library")

    monkeypatch.setattr(_lib, "load", refuse)
    module = embeddings.CharUnitEmbedder(20, 8, embeddings.CnnConfig(8, 3, 4, 2, 3), dropout_rate=0.1)
    module(torch.randint(0, 20, (6, 9))).sum().backward()
    assert all(p.grad is not None for p in module.parameters())


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert os.path.exists(B.build())
    return _lib.load()


def test_header_declares_the_new_symbols_and_lib_binds_them(lib):
    from ptgnn_amd import _lib, build as B
    assert "char_conv.hip" in B.SOURCES
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_(?:char_embed|window_)[a-z0-9_]*)\s*\(", text)))
    assert declared == SYMBOLS
    exports = open(os.path.join(ROOT, "ptgnn_amd", "csrc", "exports.map")).read()
    assert "global: ptgnn_amd_*;" in exports                      # the map exports the whole ptgnn_amd_ prefix
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "char_embed" in s or "_window_" in s) == declared
    assert sorted(_lib.SIGNATURES) == sorted(set(re.findall(r"\b(ptgnn_amd_[a-z0-9_]+)\s*\(", text)))


def test_library_still_reports_version_102_and_the_counter_lists_are_unchanged(lib):
    from ptgnn_amd import ops
    assert lib.ptgnn_amd_version() == 102
    assert list(ops.launch_counts()) == DEFAULT_COUNTERS
    agg = list(ops.launch_counts(aggregation=True))
    assert agg[:len(DEFAULT_COUNTERS)] == DEFAULT_COUNTERS and agg[-2:] == ["embedding_bag", "embedding_bag_backward"]
    assert not set(CHAR_COUNTERS) & set(agg)
    assert list(ops.launch_counts(char_cnn=True)) == DEFAULT_COUNTERS + CHAR_COUNTERS
    assert list(ops.launch_counts(aggregation=True, char_cnn=True)) == agg + CHAR_COUNTERS
    # launches_since sees every range
    before = {k: v - 1 for k, v in ops.launch_counts(aggregation=True, char_cnn=True).items()}
    assert set(ops.launches_since(before)) == set(agg + CHAR_COUNTERS)
    first = 128                                                    # the third id range starts past the aggregation range
    assert [lib.ptgnn_amd_launch_name(first + i) for i in range(5)] == [n.encode() for n in CHAR_COUNTERS] + [None]
    assert lib.ptgnn_amd_launch_count(first) == 0 and lib.ptgnn_amd_launch_count(first + 4) == -1


def test_supported_range_and_the_exported_chunk(lib):
    sup = lib.ptgnn_amd_char_embed_supported
    for chars in (0, 1, 70, 213, 214, 639, 640):
        for window in (0, 1, 3, 16, 17):
            for dim in (0, 2, 4, 6, 256, 1024, 1028):
                want = int(chars >= 1 and 1 <= window <= 16 and dim % 4 == 0 and 4 <= dim <= 1024
                           and (window * chars + 1) * 64 * 4 <= 160 * 1024)
                assert sup(chars, window, dim) == want, (chars, window, dim)
    assert sup(70, 3, 256) == 1                                    # the reference's default configuration
    assert sup(213, 3, 256) == 1 and sup(214, 3, 256) == 0         # 640 x 64 floats = one CU's LDS
    chunk = lib.ptgnn_amd_char_embed_backward_chunk()
    assert chunk >= 1
    wsb = lib.ptgnn_amd_char_embed_backward_workspace_bytes
    assert wsb(0, 70, 3, 256) == 0
    assert [wsb(n, 70, 3, 256) for n in (1, chunk, chunk + 1)] == [211 * 256 * 4, 211 * 256 * 4, 2 * 211 * 256 * 4]


def test_argument_checks_without_a_gpu(lib):
    from ptgnn_amd import _lib
    fake = ctypes.c_void_p(4096)                                   # never dereferenced: every call fails its checks first

    def embed(chars=fake, B=3, L=15, C=70, W=3, table=fake, dim=256, act=2, out=fake, ld=None):
        return lib.ptgnn_amd_char_embed_f32(chars, B, L, C, W, table, None, dim, act, out, dim if ld is None else ld, None)

    def embed_bwd(grad=fake, a1=fake, chars=fake, B=3, L=15, C=70, W=3, dim=256, act=2, gt=fake, ws=fake, ws_bytes=1 << 30):
        return lib.ptgnn_amd_char_embed_backward_f32(grad, dim, a1, dim, chars, B, L, C, W, dim, act, gt, None, ws, ws_bytes,
                                                     None)

    for fn, what in ((embed, b"char_embed"), (embed_bwd, b"char_embed_backward")):
        for bad in (dict(B=-1), dict(L=0), dict(C=0), dict(W=0), dict(dim=0), dict(W=16, L=15), dict(act=1), dict(act=3)):
            assert fn(**bad) == -1 and what in lib.ptgnn_amd_last_error(), bad
        for unsupported in (dict(dim=254), dict(dim=1028), dict(C=214), dict(W=17, L=20)):
            assert fn(**unsupported) == _lib.EUNSUPPORTED and what in lib.ptgnn_amd_last_error(), unsupported
        assert fn(chars=None) == -1 and what in lib.ptgnn_amd_last_error()
    assert embed(table=None) == -1 and embed(out=None) == -1 and embed(ld=252) == -1
    assert embed(B=0, chars=None, table=None, out=None) == 0      # nothing to do
    assert embed_bwd(grad=None) == -1 and embed_bwd(a1=None) == -1 and embed_bwd(gt=None) == -1
    assert embed_bwd(ws_bytes=211 * 256 * 4 - 1) == -4 and b"workspace" in lib.ptgnn_amd_last_error()
    assert embed_bwd(ws=None) == -4

    def wlin(x=fake, rows=10, c_in=64, window=3, ld_x=None, w=fake, n_out=32, act=2, y=fake, ld_y=32):
        return lib.ptgnn_amd_window_linear_f32(x, rows, c_in, window, c_in if ld_x is None else ld_x, w, n_out, None, act,
                                               y, ld_y, None)

    for bad in (dict(rows=-1), dict(c_in=0), dict(window=0), dict(n_out=0), dict(act=-1), dict(act=3), dict(x=None),
                dict(w=None), dict(y=None), dict(ld_y=31), dict(ld_x=63), dict(ld_x=68), dict(c_in=1 << 20, window=1 << 11)):
        assert wlin(**bad) == -1 and b"window_linear" in lib.ptgnn_amd_last_error(), bad
    assert wlin(rows=0, x=None, y=None) == 0
    # ptgnn_amd_linear_f32 keeps its own check: rows that overlap are the new entry's alone
    assert lib.ptgnn_amd_linear_f32(fake, 10, 192, 64, fake, 32, None, 0, fake, 32, None) == -1
    assert b"linear: null/ld" in lib.ptgnn_amd_last_error()

    def wgrad(x=fake, rows=10, c_in=64, window=3, g=fake, ld_g=32, n_out=32, gw=fake, ws=fake, ws_bytes=1 << 30):
        return lib.ptgnn_amd_window_weight_grad_f32(x, rows, c_in, window, g, ld_g, n_out, gw, None, ws, ws_bytes, None)

    for bad in (dict(rows=-1), dict(c_in=0), dict(window=0), dict(n_out=0), dict(x=None), dict(g=None), dict(gw=None),
                dict(ws_bytes=0)):
        assert wgrad(**bad) == -1, bad
    assert b"window_weight_grad" in lib.ptgnn_amd_last_error() or b"edge_weight_grad" in lib.ptgnn_amd_last_error()
    assert wgrad(c_in=6) == _lib.EUNSUPPORTED and wgrad(n_out=30, ld_g=32) == _lib.EUNSUPPORTED

    def wmax(x=fake, ld_x=64, B=3, R=13, valid=9, dim=64, out=fake, ld_out=64):
        return lib.ptgnn_amd_window_max_f32(x, ld_x, B, R, valid, dim, out, ld_out, None, None)

    def wmax_bwd(g=fake, ld_g=64, arg=fake, B=3, R=13, dim=64, gx=fake, ld_gx=64):
        return lib.ptgnn_amd_window_max_backward_f32(g, ld_g, arg, B, R, dim, gx, ld_gx, None)

    for bad in (dict(B=-1), dict(R=0), dict(dim=0), dict(valid=0), dict(valid=14), dict(x=None), dict(out=None),
                dict(ld_x=63), dict(ld_out=63)):
        assert wmax(**bad) == -1 and b"window_max" in lib.ptgnn_amd_last_error(), bad
    assert wmax(valid=14) == -1 and b"valid=14" in lib.ptgnn_amd_last_error()       # valid > rows_per_sample
    assert wmax(B=0, x=None, out=None) == 0
    for bad in (dict(B=-1), dict(R=0), dict(dim=0), dict(g=None), dict(arg=None), dict(gx=None), dict(ld_g=63),
                dict(ld_gx=63)):
        assert wmax_bwd(**bad) == -1 and b"window_max_backward" in lib.ptgnn_amd_last_error(), bad
    assert wmax_bwd(B=0, g=None, arg=None, gx=None) == 0


def test_ops_wrappers_refuse_host_tensors():
    from ptgnn_amd import PtgnnAmdError, ops
    chars, table, bias = torch.zeros(3, 9, dtype=torch.int64), torch.randn(3 * 10, 8), torch.randn(8)
    frame = torch.randn(3 * 7 + 4, 8)
    calls = [lambda: ops.char_embed(chars, table, bias, 3),
             lambda: ops.char_embed_backward(torch.randn(21, 8), torch.randn(21, 8), chars, 10, 3),
             lambda: ops.window_linear(frame, 2, 21, 3, torch.randn(4, 24)),
             lambda: ops.window_weight_grad(frame, 2, 21, 3, torch.randn(21, 4)),
             lambda: ops.window_max(frame, 2, 3, 7, 5),
             lambda: ops.window_max_backward(torch.randn(3, 8), torch.zeros(3, 8, dtype=torch.int32), 7)]
    for call in calls:
        with pytest.raises(PtgnnAmdError, match="must live on the GPU"):
            call()


def test_the_device_route_refuses_host_and_non_int64_chars():
    """The checks of the GPU route come before any device work, so they can be reached here through the private method."""
    from ptgnn_amd import PtgnnAmdError
    module = embeddings.CharUnitEmbedder(20, 8, embeddings.CnnConfig(8, 3, 4, 3, 3))
    device_forward = module._CharUnitEmbedder__device_forward
    for chars in (torch.zeros(2, 9, dtype=torch.int64), torch.zeros(2, 9, dtype=torch.int32)):
        with pytest.raises(PtgnnAmdError, match="CUDA int64"):
            device_forward(chars)
