"""The plain bench line (`bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR]`): it times exactly the K steps and
nothing else, and the arrays it dumps are the last timed step's output -- the same for two runs whose last timed step
reads the same minibatch, and within the parity tolerance of the CPU oracle on that minibatch's inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {name[:-4]: np.load(os.path.join(d, name)) for name in os.listdir(d)}


def test_plain_bench_line_times_only_the_steps_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from benchmarks import graph2class as G2C
    from oracle import mp_oracle as O
    from ptgnn_amd import workloads
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    # the timed steps rotate over the minibatches (step i reads minibatch i mod R): both runs end on minibatch 3
    line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", a)
    _bench("--steps", "2", "--warmup", "2", "--dump-outputs", b)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "edges/sec per MP layer" and line["unit"] == "edges/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True
    for key in ("kernels", "roofline", "repeats", "sustained", "config2", "cpu_baseline", "parity", "sharded_cfg5"):
        assert key not in line, key
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64_000_000
    got, again = _load(a), _load(b)
    assert set(got) == set(again) and all(v.dtype in (np.float32, np.float64) for v in got.values())
    for k in got:
        assert np.array_equal(got[k], again[k]), k

    last = (1 + 3 - 1) % G2C.ROTATE_MINIBATCHES
    mb = workloads.batched_graphs(48, 2500, 8, 2.2, seed=1234 + last)
    st = G2C.make_cfg3(torch.device("cpu"), last)
    assert st["N"] == line["config"]["nodes_per_minibatch"][last]
    rows = got["sampled_rows"].astype(np.int64) if "sampled_rows" in got else np.arange(st["N"])
    assert np.array_equal(got["input_node_representations"], st["cpu_x"].numpy()[rows])
    assert np.array_equal(got["node_to_graph_idx"], mb["node_to_graph_idx"].numpy().astype(np.float64))
    with torch.no_grad():
        want, _ = O.gnn_forward(st["cpu_x"], st["cpu_adj"], st["specs"], True, True)
    err = float(np.abs(got["output_node_representations"] - want.numpy()[rows]).max())
    assert err <= 1e-5, err
