"""The MLP-MP layer's message GEMM and whole layer forward with fp32 against 16-bit matrix inputs (ptgnn_amd/precision.py,
`mlp=True`) in one process, at two shapes:

  * cfg2 (benchmarks/synthetic.py: N = 200k, E = 1.1M, H = M = 128, T = 1, sum): the table form -- the [N, 2 T M] table
    Linear, fp32 `ops.linear` against `ptgnn_amd_half_linear`;
  * a cfg4-like layer (N = 80k, T = 21 edge types, E = 200k, H = M = 64, max): the edge form -- the grouped per-edge GEMM
    over [x[src] | x[dst]], fp32 `ops.edge_linear` against `ptgnn_amd_edge_dst_linear16` (csrc/edge_gemm16.hip), and
    `--wide`: the same graph at H = M = 128 (the weight-stationary kernel's other register budget) and at H = 96 (the
    per-wave kernel).

Kernels alone: three interleaved repeats of `--steps` launches per mode, one HIP-event bracket per repeat, medians, next
to the HBM floor of the 16-bit launch at 8 TB/s.  Layer forward: the same under `matrix_inputs(dtype, mlp=True)` with
wall-clock per step.  The record behind profiles/mlp_inputs_notes.md:

    python -m benchmarks.mlp_inputs [--out profiles/mlp_inputs_bench.json] [--steps 10] [--wide]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from benchmarks.edge_inputs import HBM_BYTES_PER_S, interleaved, with_env
from ptgnn_amd import ops

DEV = torch.device("cuda")
MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))


def make_edge_layer(n=80_000, types=21, edges=200_000, hidden=64, reduce="max", seed=4321):
    from ptgnn_amd import layers as L, workloads
    torch.manual_seed(seed)
    layer = L.MlpMessagePassingLayer(hidden, hidden, hidden, types, reduce).to(DEV).eval()
    g = torch.Generator().manual_seed(seed)
    sizes = torch.multinomial(torch.ones(types), edges, replacement=True, generator=g).bincount(minlength=types)
    adj = [(torch.randint(0, n, (int(c),), generator=g).to(DEV), torch.randint(0, n, (int(c),), generator=g).to(DEV))
           for c in sizes.tolist()]
    x = workloads.node_states(n, hidden, seed=seed).to(DEV)
    assert L._prefer_edge_path(edges, n, types, hidden, hidden)
    return {"layer": layer, "adj": adj, "x": x, "N": n, "E": edges, "H": hidden, "T": types,
            "desc": f"cfg4-like: N={n} E={edges} T={types}, 1 MLP-MP layer H=M={hidden}, {reduce}, edge form"}


def step(st):
    ops.clear_plan_cache()
    with torch.no_grad():
        return st["layer"](st["x"], st["adj"], None, {}, {}, [None] * len(st["adj"]))


def table_gemm_alone(st, steps):
    layer, x = st["layer"], st["x"]
    w = layer._stacked_edge_weights()
    n_out, k = w.shape
    rows = x.shape[0]
    rounded = {dt: w.to(dt).contiguous() for _, dt in MODES[1:]}
    with torch.no_grad():
        fns = {"float32": lambda: ops.linear(x, w)}
        for name, dt in MODES[1:]:
            fns[name] = (lambda dt: lambda: ops.linear(x, w, inputs=dt, rounded=rounded[dt]))(dt)
        res = {"shape": f"rows={rows} K={k} n_out={n_out}", "launches": interleaved(fns, steps)}
    res["hbm_floor_ms_16bit"] = round((rows * (k + n_out) * 4 + n_out * k * 2) / HBM_BYTES_PER_S * 1e3, 5)
    return _ratios(res)


def edge_gemm_alone(st, steps):
    layer, x, adj = st["layer"], st["x"], st["adj"]
    ws = [w.detach() for w in layer._first_weights()]
    T, (M, K) = len(ws), ws[0].shape
    E, H = st["E"], st["H"]
    stacks = {dt: torch.stack(ws).to(dt).contiguous() for _, dt in MODES[1:]}
    with torch.no_grad():
        fns = {"float32": lambda: ops.edge_linear(x, adj, ws, True)}
        for name, dt in MODES[1:]:
            fns[name] = (lambda dt: lambda: ops.edge_linear(x, adj, ws, True, inputs=dt, rounded=stacks[dt]))(dt)
        before = ops.launch_counts(edge16_dst=True)
        fns["bfloat16"]()
        assert ops.launches_since(before).get("edge16_dst") == 1
        res = {"shape": f"E={E} H={H} M={M} T={T}", "launches": interleaved(fns, steps)}
        # developer A/B knobs of csrc/edge_gemm16.hip, read per launch: the per-wave kernel in the weight-stationary
        # one's place, and other workgroup counts per CU than one resident round
        res["variants_bfloat16"] = interleaved(
            {"float32": fns["float32"], "default": fns["bfloat16"],
             "per_wave": with_env({"PTGNN_AMD_EDGE16_WS": "0"}, fns["bfloat16"]),
             **{f"ws_{n}_per_cu": with_env({"PTGNN_AMD_EDGE16_WGS": str(n)}, fns["bfloat16"]) for n in (2, 4, 8)}},
            steps)
    # every message row gathers two fp32 state rows and writes one fp32 message row; ids 16 bytes; 16-bit weights
    res["hbm_floor_ms_16bit"] = round((E * (2 * H + M) * 4 + E * 16 + T * M * K * 2) / HBM_BYTES_PER_S * 1e3, 5)
    return _ratios(res)


def _ratios(res):
    med = {k: v["median_ms"] for k, v in res["launches"].items()}
    for name in ("bfloat16", "float16"):
        res[f"{name}_over_fp32"] = round(med[name] / med["float32"], 4)
        res[f"{name}_over_hbm_floor"] = round(med[name] / res["hbm_floor_ms_16bit"], 3)
    res["float32_over_hbm_floor_16bit"] = round(med["float32"] / res["hbm_floor_ms_16bit"], 3)
    return res


def forward_modes(step_fn, steps, repeats=3):
    for _, dt in MODES:                               # warm-up: every mode, plan caches, allocator
        with ptgnn_amd.matrix_inputs(dt, mlp=True):
            for _ in range(2):
                step_fn()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _ in MODES}
    for _ in range(repeats):
        for name, dt in MODES:
            with ptgnn_amd.matrix_inputs(dt, mlp=True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step_fn()
                torch.cuda.synchronize()
                out[name]["ms_per_step"].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
                timer = ops.KernelTimer()
                ops.set_kernel_timer(timer)
                for _ in range(steps):
                    step_fn()
                ops.set_kernel_timer(None)
                for k, v in timer.summary().items():
                    out[name]["kernels"].setdefault(k, []).append(round(v["ms"] / v["calls"], 5))
    for rec in out.values():
        rec["ms_per_step_median"] = statistics.median(rec["ms_per_step"])
        rec["kernels_median_ms"] = {k: statistics.median(v) for k, v in rec.pop("kernels").items()}
    f32 = out["float32"]["ms_per_step_median"]
    return {"modes": out, **{f"{name}_over_fp32": round(out[name]["ms_per_step_median"] / f32, 4)
                             for name, _ in MODES[1:]}}


def main(out=None, steps=10, wide=False):
    from benchmarks import synthetic
    res = {"device": torch.cuda.get_device_name(0),
           "timing": f"3 interleaved repeats of {steps} launches (kernels) / steps (forward) per mode, medians"}
    st = synthetic.make_cfg2(DEV, 0, 1)
    res["cfg2"] = {"workload": st["desc"], "table_gemm_alone": table_gemm_alone(st, steps),
                   "layer_forward": forward_modes(lambda: synthetic.step_cfg2(st, 1), steps)}
    del st
    torch.cuda.empty_cache()
    for key, hidden in (("cfg4_like", 64),) + ((("cfg4_like_h128", 128), ("cfg4_like_h96", 96)) if wide else ()):
        st = make_edge_layer(hidden=hidden)
        res[key] = {"workload": st["desc"], "edge_gemm_alone": edge_gemm_alone(st, steps),
                    "layer_forward": forward_modes(lambda: step(st), steps)}
        del st
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/mlp_inputs_bench.json")
    parser.add_argument("--steps", type=int, default=10)
    parser.add_argument("--wide", action="store_true")
    args = parser.parse_args()
    main(args.out, args.steps, args.wide)
