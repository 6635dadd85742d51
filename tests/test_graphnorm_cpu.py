"""GraphNorm on host tensors (ptgnn_amd.torch_route.graph_norm) against fixtures of the reference's own class in fp32 and
float64 (tests/golden/make_golden_graphnorm.py), its state_dict, the refusal of `forward_sharded`, the C ABI of
csrc/graph_norm.hip and -- where the reference is mounted -- the live reference inside its own container."""
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
from graphnorm_cases import CASES, COUNTS, NUM_GRAPHS, build
from oracle import shims
from ptgnn_amd import layers as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IDS = [name for name, _ in CASES]
PARAMS = ("gamma", "alpha", "bias")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def ok(got, want32, want64):
    want64 = torch.as_tensor(want64)
    return attributed_ok(got, torch.as_tensor(want32), want64, tol=TOL, scale=max(1.0, float(want64.abs().max())))


def test_fixtures_cover_widths_parameters_eps_and_graph_shapes():
    specs = [spec for _, spec in CASES]
    assert {s["D"] for s in specs} == {6, 64}
    assert {s["random_params"] for s in specs} == {True, False}
    assert {s["eps"] for s in specs} == {1e-10, 1e-5}
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("graphnorm_"))
    for name, spec in CASES:
        fx = load(name)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= largest
        assert json.loads(str(fx["spec"])) == spec
        idx = fx["index"]
        assert int(idx.max()) + 1 == NUM_GRAPHS
        assert np.bincount(idx, minlength=NUM_GRAPHS).tolist() == COUNTS       # 70, 1, 0, 33, 2, an empty graph, 1
        assert not bool((idx[1:] >= idx[:-1]).all())                             # unsorted map
        assert fx["x"].dtype == np.float32 and fx["y64"].dtype == np.float64
        state = state_of(fx)
        assert list(state) == list(PARAMS)
        default = bool((state["alpha"] == 1).all() and (state["gamma"] == 1).all() and (state["bias"] == 0).all())
        assert default == (not spec["random_params"])
        if spec["random_params"]:
            for k in ("gamma", "alpha"):
                assert 0.5 <= float(state[k].min()) and float(state[k].max()) <= 1.5
        for k in ("x",) + PARAMS:
            assert fx["grad." + k].dtype == np.float32 and fx["grad64." + k].dtype == np.float64


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_output_and_gradients_match_the_reference(name, spec):
    fx = load(name)
    layer = build(spec, L)
    layer.load_state_dict(state_of(fx), strict=True)
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    y = layer(x, [], torch.from_numpy(fx["index"]), {}, {}, [])
    assert y.shape == x.shape and y.dtype == torch.float32 and not y.is_cuda
    assert ok(y, fx["y"], fx["y64"])
    (y * torch.from_numpy(fx["gout"])).sum().backward()
    assert ok(x.grad, fx["grad.x"], fx["grad64.x"])
    for k, p in layer.named_parameters():
        assert ok(p.grad, fx["grad." + k], fx["grad64." + k]), k


def test_state_dict_keys_shapes_initial_values_and_properties():
    layer = L.GraphNorm(input_state_dimension=12)
    sd = layer.state_dict()
    assert list(sd) == list(PARAMS)
    assert all(tuple(v.shape) == (1, 12) for v in sd.values())
    assert torch.equal(sd["gamma"], torch.ones(1, 12)) and torch.equal(sd["alpha"], torch.ones(1, 12))
    assert torch.equal(sd["bias"], torch.zeros(1, 12))
    assert [k for k, _ in layer.named_parameters()] == list(PARAMS)
    assert layer.input_state_dimension == 12 and layer.output_state_dimension == 12
    assert isinstance(layer, L.AbstractMessagePassingLayer)
    assert L.GraphNorm(5, eps=1e-3).input_state_dimension == 5


@pytest.mark.parametrize("name,spec", CASES[:2], ids=IDS[:2])
def test_fixture_state_round_trips_strictly(name, spec):
    want = state_of(load(name))
    layer = build(spec, L)
    res = layer.load_state_dict(want, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in layer.state_dict().items():
        assert torch.equal(v, want[k]), k
    again = build(spec, L)
    again.load_state_dict(layer.state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        again.load_state_dict({k: v for k, v in want.items() if k != "alpha"}, strict=True)


def test_eps_is_used():
    x = torch.zeros(3, 4)
    idx = torch.zeros(3, dtype=torch.int64)
    x[0, 0] = 1.0
    with torch.no_grad():
        y_small = L.GraphNorm(4, eps=1e-10)(x, [], idx, {}, {}, [])
        y_big = L.GraphNorm(4, eps=1.0)(x, [], idx, {}, {}, [])
    assert float(y_small[0, 0]) > 1.0 > float(y_big[0, 0]) > 0.0
    assert float(y_small[:, 1:].abs().max()) == 0.0                              # 0 / sqrt(eps) = 0: no NaN


def test_forward_sharded_raises():
    layer = L.GraphNorm(8)
    with pytest.raises(NotImplementedError, match="span ranks"):
        layer.forward_sharded(torch.randn(4, 8), None)
    from ptgnn_amd import sharded  # noqa: F401  (run_stack dispatches on the attribute)
    assert hasattr(layer, "forward_sharded")


def test_header_exports_and_signatures_agree_on_the_graph_norm_entry_points():
    from ptgnn_amd import _lib, build as B
    assert "graph_norm.hip" in B.SOURCES
    path = B.build()
    text = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    assert "graphnorm.py:36-46" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_graph_norm_[a-z0-9_]+)\s*\(", code)))
    assert declared == ["ptgnn_amd_graph_norm_backward_f32", "ptgnn_amd_graph_norm_backward_workspace_bytes",
                        "ptgnn_amd_graph_norm_f32", "ptgnn_amd_graph_norm_supported",
                        "ptgnn_amd_graph_norm_workspace_bytes"]
    raw = ctypes.CDLL(path)
    for s in declared:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert sorted(s for s in _lib.SIGNATURES if "graph_norm" in s) == declared
    lib = _lib.load()
    assert lib.ptgnn_amd_version() == 102
    assert [lib.ptgnn_amd_graph_norm_supported(d) for d in (0, 1, 64, 1024, 1025)] == [0, 1, 1, 1, 0]
    assert lib.ptgnn_amd_graph_norm_workspace_bytes(5, 1000, 64) > 0
    assert lib.ptgnn_amd_graph_norm_backward_workspace_bytes(5, 1000, 64) > 0
    # bad arguments are refused before any HIP call
    rc = lib.ptgnn_amd_graph_norm_f32(None, 4, None, None, None, 1e-5, None, None, 1, 0, 2000, None, 4, None, None, 0, None)
    assert rc == _lib.EUNSUPPORTED and b"graph_norm" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_graph_norm_f32(None, 4, None, None, None, 1e-5, None, None, 1, 0, 4, None, 4, None, None, 0, None)
    assert rc == -1 and b"graph_norm" in lib.ptgnn_amd_last_error()
    rc = lib.ptgnn_amd_graph_norm_backward_f32(None, 4, None, 4, None, None, 1e-5, None, None, None, 1, 0, 4, None, 4, None,
                                               None, None, None, 0, None)
    assert rc == -1 and b"graph_norm_backward" in lib.ptgnn_amd_last_error()


def test_launch_counter_families_are_listed():
    from ptgnn_amd import ops
    counts = ops.launch_counts(aggregation=True)
    assert "graph_norm" in counts and "graph_norm_backward" in counts
    assert "graph_norm" not in ops.launch_counts()
    assert ops.launches_since(counts) == {}


def test_c_abi_wrappers_refuse_host_tensors():
    from ptgnn_amd import PtgnnAmdError, ops
    with pytest.raises(PtgnnAmdError):
        ops.graph_norm(torch.randn(4, 8), torch.ones(8), torch.ones(8), torch.zeros(8), 1e-5, None)


@pytest.mark.skipif(not shims.reference_available(), reason="reference checkout not mounted")
def test_live_reference_exchanges_state_and_agrees_inside_its_container():
    """tests/graphnorm_dropin_check.py in a fresh interpreter (the reference's shims stay out of this process)."""
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "graphnorm_dropin_check.py")],
                          env=dict(os.environ, PYTHONHASHSEED="0"), capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "GRAPHNORM_DROPIN_OK" in proc.stdout
