"""MultiHeadSelfAttentionMessagePassing on host tensors (ptgnn_amd.torch_route.self_attention_message_passing) against
fixtures of the reference's own class in fp32 and float64 (tests/golden/make_golden_selfatt.py), its state_dict, the
window rule, the refusals, the C ABI of csrc/block_attention.hip and -- where the reference is mounted -- the live
reference inside its own container."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from agg_paths import TOL, attributed_ok
from oracle import shims
from ptgnn_amd import PtgnnAmdError, layers as L
from selfatt_cases import CASES, GOLDEN, STATE_KEYS, TARGET, build, call, files, load, sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [name for name, _ in CASES]


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def ok(got, want32, want64):
    want64 = torch.as_tensor(want64)
    return attributed_ok(got, torch.as_tensor(want32), want64, tol=TOL, scale=max(1.0, float(want64.abs().max())))


def test_fixtures_cover_the_cases_and_graph_shapes():
    specs = [spec for _, spec in CASES]
    assert sorted((s["D"], s["dk"], s["dv"], s["heads"], s["max"]) for s in specs if not s["target"]) == \
        [(32, 6, 10, 3, 40), (32, 8, 8, 4, 40), (64, 32, 32, 8, 40), (64, 64, 64, 2, 250)]
    assert [s["scale"] for s in specs if (s["D"], s["dk"]) == (32, 8) and not s["target"]] == [6.0]
    assert sum(s["target"] for s in specs) == 1 and sum(s["unsorted"] for s in specs) >= 2
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("selfatt_"))
    for name, spec in CASES:
        for path in files(name):
            assert os.path.getsize(path) <= min(largest, 1 << 20), path
        fx = load(name)
        assert json.loads(str(fx["spec"])) == spec
        idx = fx["index"]
        assert np.bincount(idx).tolist() == sizes(spec["max"])
        assert bool((idx[1:] >= idx[:-1]).all()) == (not spec["unsorted"])
        assert fx["x"].dtype == np.float32 and fx["y64"].dtype == np.float64
        assert list(state_of(fx)) == STATE_KEYS
        if spec["target"]:
            assert sorted(fx["ids"].tolist()) == list(range(idx.shape[0]))
            assert fx["ids"].tolist() != list(range(idx.shape[0]))
        for k in ["x"] + STATE_KEYS:
            assert fx["grad." + k].dtype == np.float32 and fx["grad64." + k].dtype == np.float64


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_output_and_gradients_match_the_reference(name, spec):
    fx = load(name)
    layer = build(spec, L).eval()
    layer.load_state_dict(state_of(fx), strict=True)
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    y = call(layer, spec, x, fx["index"], fx.get("ids"))
    assert y.shape == x.shape and y.dtype == torch.float32 and not y.is_cuda
    assert ok(y, fx["y"], fx["y64"])
    (y * torch.from_numpy(fx["gout"])).sum().backward()
    assert ok(x.grad, fx["grad.x"], fx["grad64.x"])
    for k, p in layer.named_parameters():
        assert ok(p.grad, fx["grad." + k], fx["grad64." + k]), k


def test_cpu_route_in_float64_matches_the_float64_fixture():
    name, spec = CASES[0]
    fx = load(name)
    layer = build(spec, L).eval()
    layer.load_state_dict(state_of(fx), strict=True)
    y = call(layer.double(), spec, torch.from_numpy(fx["x"]).double(), fx["index"])
    assert y.dtype == torch.float64 and float((y - torch.from_numpy(fx["y64"])).abs().max()) < 1e-12


def test_state_dict_keys_order_properties_and_defaults():
    layer = L.MultiHeadSelfAttentionMessagePassing(12, 5, 7, 12, 20, 3)
    assert list(layer.state_dict()) == STATE_KEYS
    sd = layer.state_dict()
    assert tuple(sd[STATE_KEYS[0]].shape) == (3 * (2 * 5 + 7), 12) and tuple(sd[STATE_KEYS[1]].shape) == (12, 21)
    assert layer.input_state_dimension == 12 and layer.output_state_dimension == 12
    assert isinstance(layer, L.AbstractMessagePassingLayer)
    import inspect
    sig = inspect.signature(L.MultiHeadSelfAttentionMessagePassing.__init__)
    assert list(sig.parameters)[1:] == ["input_state_dimension", "key_query_dimension", "value_dimension",
                                        "output_dimension", "intermediate_dimension", "num_heads", "dropout_rate",
                                        "target_reference", "max_num_nodes"]
    assert (sig.parameters["dropout_rate"].default, sig.parameters["target_reference"].default,
            sig.parameters["max_num_nodes"].default) == (0.0, "all", 250)


@pytest.mark.parametrize("name,spec", CASES[:2], ids=IDS[:2])
def test_fixture_state_round_trips_strictly(name, spec):
    want = state_of(load(name))
    layer = build(spec, L)
    res = layer.load_state_dict(want, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(layer.state_dict()) == STATE_KEYS
    for k, v in layer.state_dict().items():
        assert torch.equal(v, want[k]), k
    again = build(spec, L)
    again.load_state_dict(layer.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        again.load_state_dict({k: v for k, v in want.items() if k != STATE_KEYS[1]}, strict=True)


def test_unsorted_map_equals_its_sorted_form_bit_for_bit():
    name, spec = CASES[0]
    fx = load(name)
    layer = build(spec, L).eval()
    layer.load_state_dict(state_of(fx), strict=True)
    x = torch.from_numpy(fx["x"])
    idx = torch.from_numpy(fx["index"])
    assert not bool((idx[1:] >= idx[:-1]).all())
    with torch.no_grad():
        assert torch.equal(layer(x, [], idx, {}, {}, []), layer(x, [], idx.sort().values, {}, {}, []))


def test_windows_are_runs_of_rows_cut_every_max_num_nodes():
    from ptgnn_amd import torch_route
    idx = torch.tensor([3, 0, 0, 5, 3, 3, 0, 5, 5, 5, 5])          # counts 3, 0, 0, 3, 0, 5
    assert torch_route.attention_window_bounds(idx, 2) == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 8), (8, 10), (10, 11)]
    assert torch_route.attention_window_bounds(idx, 250) == [(0, 3), (3, 6), (6, 11)]
    assert torch_route.attention_window_bounds(idx[:0], 4) == []


def test_partial_target_reference_raises_naming_line_119():
    layer = L.MultiHeadSelfAttentionMessagePassing(8, 2, 2, 8, 8, 2, target_reference=TARGET)
    x = torch.randn(6, 8)
    with pytest.raises(PtgnnAmdError, match="119"):
        layer(x, [], torch.zeros(6, dtype=torch.int64), {TARGET: torch.tensor([0, 3])}, {TARGET: torch.tensor([0, 0])}, [])


def test_target_reference_does_not_mutate_the_input():
    name, spec = CASES[-1]
    fx = load(name)
    layer = build(spec, L).eval()
    layer.load_state_dict(state_of(fx), strict=True)
    x = torch.from_numpy(fx["x"])
    keep = x.clone()
    with torch.no_grad():
        y = call(layer, spec, x, fx["index"], fx["ids"])
    assert torch.equal(x, keep) and y.data_ptr() != x.data_ptr()


def test_forward_sharded_raises():
    layer = L.MultiHeadSelfAttentionMessagePassing(8, 2, 2, 8, 8, 2)
    with pytest.raises(NotImplementedError, match="span ranks"):
        layer.forward_sharded(torch.randn(4, 8), None)


def test_header_exports_and_signatures_agree_on_the_block_attention_entry_points():
    from ptgnn_amd import _lib, build as B
    assert "block_attention.hip" in B.SOURCES
    path = B.build()
    text = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    assert "selfattmessagepassing.py:59-75" in text and "selfattmessagepassing.py:104-117" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_(?:block_attention|attention_windows)[a-z0-9_]*)\s*\(", code)))
    assert declared == ["ptgnn_amd_attention_windows", "ptgnn_amd_attention_windows_bound",
                        "ptgnn_amd_block_attention_backward_f32", "ptgnn_amd_block_attention_backward_workspace_bytes",
                        "ptgnn_amd_block_attention_f32", "ptgnn_amd_block_attention_supported"]
    raw = ctypes.CDLL(path)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "block_attention" in s or "attention_windows" in s) == declared
    lib = _lib.load()
    assert lib.ptgnn_amd_version() == 102
    assert [lib.ptgnn_amd_block_attention_supported(d, d) for d in (0, 1, 128, 129)] == [0, 1, 1, 0]
    assert lib.ptgnn_amd_block_attention_supported(128, 129) == 0 and lib.ptgnn_amd_block_attention_supported(129, 1) == 0
    assert lib.ptgnn_amd_attention_windows_bound(7, 236, 40) == 6 + 7 and lib.ptgnn_amd_attention_windows_bound(1, 1, 0) == -1
    assert lib.ptgnn_amd_block_attention_backward_workspace_bytes(1000, 8) >= 32000
    # bad arguments are refused before any HIP call
    rc = lib.ptgnn_amd_block_attention_f32(None, 96, None, 3, 10, 40, 1, 32, 32, 0.0, 0, None, 32, None, None)
    assert rc == -1 and b"block_attention" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_block_attention_f32(None, 96, None, 3, 10, 40, 1, 129, 32, 0.0, 0, None, 32, None, None)
    assert rc == _lib.EUNSUPPORTED and b"block_attention" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_block_attention_backward_f32(None, 96, None, 32, None, None, 32, None, 3, 10, 40, 1, 32, 32, 0.0, 0,
                                                    None, 96, None, 0, None)
    assert rc == -1 and b"block_attention_backward" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_attention_windows(None, 3, 10, 40, None, 5, None)
    assert rc == -1 and b"block_attention" in lib.ptgnn_amd_last_error()


def test_launch_counter_families_are_listed_under_aggregation_only():
    from ptgnn_amd import ops
    counts = ops.launch_counts(aggregation=True)
    assert "block_attention" in counts and "block_attention_backward" in counts
    assert "block_attention" not in ops.launch_counts() and "block_attention_backward" not in ops.launch_counts()
    assert ops.launches_since(counts) == {}
    assert ops.BLOCK_ATTENTION_COL_TILE == 32 and ops.BLOCK_ATTENTION_ROW_TILES == (32, 64, 128)


def test_c_abi_wrappers_refuse_host_tensors():
    from ptgnn_amd import ops
    with pytest.raises(PtgnnAmdError):
        ops.block_attention(torch.randn(4, 12), torch.zeros(2, dtype=torch.int32), 4, 1, 4, 4)


@pytest.mark.skipif(not shims.reference_available(), reason="reference checkout not mounted")
def test_live_reference_exchanges_state_and_agrees_inside_its_container():
    """tests/selfatt_dropin_check.py in a fresh interpreter (the reference's shims stay out of this process)."""
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "selfatt_dropin_check.py")],
                          env=dict(os.environ, PYTHONHASHSEED="0"), capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "SELFATT_DROPIN_OK" in proc.stdout
