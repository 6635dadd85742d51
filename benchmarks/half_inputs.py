"""GGNN inference forward with fp32 against bf16 matrix inputs (ptgnn_amd/precision.py) in one process, at the cfg3 and
cfg5 layer shapes: per mode three repeats, interleaved (fp32, bf16, fp32, ...), after a warm-up of both; per-kernel
HIP-event times from `ops.KernelTimer`, wall time per step from a synchronised block.  Also the two dense blocks alone
at the cfg3 shape (the cfg3 batch takes the edge form, so its table Linear is timed on its own).  The record behind
profiles/half_inputs_notes.md:

    python -m benchmarks.half_inputs [--out profiles/half_inputs_bench.json] [--steps 5]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from ptgnn_amd import ops

DEV = torch.device("cuda")
MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
DENSE = ("linear", "gru_cell", "half_linear", "half_gru_cell", "edge_linear", "edge_linear_shared")


def measure(step, steps, repeats=3):
    """{mode: {"ms_per_step": [per repeat], "kernels": {name: [avg ms per call, per repeat]}}}"""
    for _, dt in MODES:                              # warm-up: both modes, plan caches, allocator
        with ptgnn_amd.matrix_inputs(dt):
            for _ in range(2):
                step()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _ in MODES}
    for _ in range(repeats):
        for name, dt in MODES:
            with ptgnn_amd.matrix_inputs(dt):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                out[name]["ms_per_step"].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                for _ in range(steps):
                    step()
                ops.set_kernel_timer(None)
                for k, v in timer.summary().items():
                    out[name]["kernels"].setdefault(k, []).append(round(v["ms"] / v["calls"], 5))
    for rec in out.values():
        rec["ms_per_step_median"] = statistics.median(rec["ms_per_step"])
        rec["kernels_median_ms"] = {k: statistics.median(v) for k, v in rec["kernels"].items()}
    return out


def events(fn, reps=20):
    for _ in range(3):
        fn()
    evs = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in evs), 5)


def dense_alone(n, m, hd, n_out):
    """The GRU cell and the table Linear alone on [n, .] fp32 states: median of 20 HIP-event brackets per mode, and the
    HBM floor of the 16-bit kernels at 8 TB/s (GRU: n (m + 2 hd) 4 bytes; Linear: n (k + n_out) 4 bytes)."""
    g = torch.Generator().manual_seed(1)
    a, h = torch.randn(n, m, generator=g).to(DEV), torch.randn(n, hd, generator=g).to(DEV)
    gru = torch.nn.GRUCell(m, hd).to(DEV)
    w = (torch.randn(n_out, hd, generator=g) * 0.05).to(DEV)
    p = [t.detach() for t in (gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh)]
    res = {"shape": f"n={n} m={m} hd={hd} n_out={n_out}",
           "gru_hbm_floor_ms": round(n * (m + 2 * hd) * 4 / 8e12 * 1e3, 5),
           "linear_hbm_floor_ms": round(n * (hd + n_out) * 4 / 8e12 * 1e3, 5)}
    with torch.no_grad():
        for name, dt in MODES:
            res[f"gru_cell_ms_{name}"] = events(lambda: ops.gru_cell(a, h, *p, inputs=dt))
            res[f"linear_ms_{name}"] = events(lambda: ops.linear(h, w, inputs=dt))
    res["gru_ratio_bf16_over_fp32"] = round(res["gru_cell_ms_bfloat16"] / res["gru_cell_ms_float32"], 4)
    res["linear_ratio_bf16_over_fp32"] = round(res["linear_ms_bfloat16"] / res["linear_ms_float32"], 4)
    return res


def ratios(rec):
    f, b = rec["float32"]["kernels_median_ms"], rec["bfloat16"]["kernels_median_ms"]
    out = {"step": round(rec["bfloat16"]["ms_per_step_median"] / rec["float32"]["ms_per_step_median"], 4)}
    if "gru_cell" in f and "half_gru_cell" in b:
        out["half_gru_cell_over_gru_cell"] = round(b["half_gru_cell"] / f["gru_cell"], 4)
    if "linear" in f and "half_linear" in b:
        out["half_linear_over_linear"] = round(b["half_linear"] / f["linear"], 4)
    return out


def main(out=None, steps=5):
    from benchmarks import graph2class as G2C
    from ptgnn_amd import layers as L, workloads
    res = {"device": torch.cuda.get_device_name(0), "timing": f"3 interleaved repeats of {steps} steps per mode"}

    st = G2C.make_cfg3(DEV)
    rec = measure(lambda: G2C.step_cfg3(st), steps)
    res["cfg3"] = {"workload": st["desc"], "modes": rec, "bf16_over_fp32": ratios(rec)}
    n3 = st["N"]
    del st
    torch.cuda.empty_cache()
    res["cfg3_dense_alone"] = dense_alone(n3, 128, 128, 17 * 128)

    N, E, H = 1_250_000, 12_500_000, 256
    adj = workloads.power_law_graph(N, E, alpha=0.8, seed=1234)
    cadj = [(adj[0][0].to(DEV), adj[0][1].to(DEV))]
    x = workloads.node_states(N, H, seed=2).to(DEV)
    torch.manual_seed(5)
    layer = L.GatedMessagePassingLayer(H, H, 1, "sum").eval().to(DEV)

    def step5():
        ops.clear_plan_cache()
        with torch.no_grad():
            return layer(x, cadj, None, {}, {}, [None])
    rec = measure(step5, max(2, steps // 2))
    res["cfg5"] = {"workload": f"cfg5 per-GPU shard: power-law N={N} E={E}, 1 GGNN layer H=M={H}, sum (table form)",
                   "modes": rec, "bf16_over_fp32": ratios(rec)}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/half_inputs_bench.json")
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    main(args.out, args.steps)
