"""SelfAttentionVarSizedElementReduce / MultiheadSelfAttentionVarSizedElementReduce on host tensors
(ptgnn_amd.torch_route.attention_summary) against fixtures of the reference's own classes
(tests/golden/make_golden_attnpool.py): state_dict keys, same-seed initial parameters, outputs and gradients."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from attnpool_cases import CASES, NUM_SAMPLES, SIZES, build
from oracle import shims
from ptgnn_amd import reduceops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-6
# a parameter gradient adds one fp32 term per element (185 here) in the backward of the scatter: the restated
# torch_scatter of the fixtures and the host route add them in different orders (up to 2.6e-6 of the largest entry)
PARAM_TOL = 5e-6
IDS = [name for name, _ in CASES]


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def close(got, want, tol=TOL):
    want = torch.as_tensor(want)
    return float((got.detach().double() - want.double()).abs().max()) <= tol * max(1.0, float(want.abs().max()))


def test_fixtures_cover_both_classes_heads_queries_and_sample_shapes():
    specs = [spec for _, spec in CASES]
    assert {s["cls"] for s in specs} == {"single", "multi"}
    assert {s["heads"] for s in specs if s["cls"] == "multi"} >= {1, 4, 8}
    assert {s["value"] for s in specs if s["cls"] == "multi"} == {True, False}
    assert {s["query"] if isinstance(s["query"], str) else "nested" for s in specs} == {"max", "mean", "wsum", "nested"}
    assert any(s["hidden"] != s["D"] for s in specs)
    for name, spec in CASES:
        fx = load(name)
        assert json.loads(str(fx["spec"])) == spec
        idx = fx["index"]
        counts = np.bincount(idx, minlength=int(fx["num_samples"]))
        assert int(fx["num_samples"]) == NUM_SAMPLES > int(idx.max()) + 1
        assert not bool((idx[1:] >= idx[:-1]).all())                      # unsorted map
        assert sorted(counts.tolist()) == sorted(SIZES + [0])
        assert counts.max() > 128 and 1 in counts.tolist() and (counts == 0).sum() == 2


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_state_dict_keys_and_same_seed_initial_parameters_match_the_reference(name, spec):
    want = state_of(load(name))
    torch.manual_seed(spec["seed"])
    module = build(spec, reduceops)
    assert list(module.state_dict()) == list(want)               # mangled names, creation order
    for k, v in module.state_dict().items():
        assert torch.equal(v, want[k]), k
    fresh = build(spec, reduceops)
    fresh.load_state_dict(want, strict=True)


@pytest.mark.parametrize("name,spec", CASES, ids=IDS)
def test_cpu_route_output_and_gradients_match_the_reference(name, spec):
    fx = load(name)
    module = build(spec, reduceops)
    module.load_state_dict(state_of(fx), strict=True)
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    y = module(reduceops.ElementsToSummaryRepresentationInput(x, torch.from_numpy(fx["index"]), NUM_SAMPLES))
    assert y.shape == (NUM_SAMPLES, spec["out"]) and not y.is_cuda
    assert close(y, fx["y"])
    (y * torch.from_numpy(fx["gout"])).sum().backward()
    assert close(x.grad, fx["grad.x"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k], PARAM_TOL), k


def test_duck_typed_input_and_tensor_num_samples():
    name, spec = CASES[2]
    fx = load(name)
    module = build(spec, reduceops)
    module.load_state_dict(state_of(fx), strict=True)
    x, idx = torch.from_numpy(fx["x"]), torch.from_numpy(fx["index"])
    duck = types.SimpleNamespace(element_embeddings=x, element_to_sample_map=idx,
                                 num_samples=torch.tensor(NUM_SAMPLES))
    assert close(module(duck), fx["y"])


def test_value_layer_and_head_count_checks_follow_the_reference():
    with pytest.raises(AssertionError):
        reduceops.MultiheadSelfAttentionVarSizedElementReduce(8, 10, 4, 4, reduceops.SimpleVarSizedElementReduce("max"))
    m = reduceops.MultiheadSelfAttentionVarSizedElementReduce(8, 8, 4, 2, reduceops.SimpleVarSizedElementReduce("max"))
    assert tuple(m.state_dict()["_MultiheadSelfAttentionVarSizedElementReduce__output_layer.weight"].shape) == (4, 16)


_LIVE = """
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import shims
shims.install()
import numpy as np, torch
from ptgnn.neuralmodels.reduceops import varsizedsummary as ref
from attnpool_cases import CASES, build
out = {}
for name, spec in CASES:
    torch.manual_seed(spec["seed"])
    for k, v in build(spec, ref).state_dict().items():
        out[name + "/" + k] = v.numpy()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.skipif(not shims.reference_available(), reason="reference checkout not mounted")
def test_same_seed_initial_parameters_equal_the_live_reference(tmp_path):
    """The reference's own constructors in a fresh interpreter (its shims stay out of this process)."""
    path = str(tmp_path / "ref_state.npz")
    proc = subprocess.run([sys.executable, "-c", _LIVE, ROOT, os.path.join(ROOT, "tests"), path],
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-3000:]
    ref_state = np.load(path)
    for name, spec in CASES:
        torch.manual_seed(spec["seed"])
        ours = build(spec, reduceops).state_dict()
        keys = sorted(k[len(name) + 1:] for k in ref_state.files if k.startswith(name + "/"))
        assert keys == sorted(ours)
        for k in keys:
            assert torch.equal(ours[k], torch.from_numpy(ref_state[name + "/" + k])), (name, k)
