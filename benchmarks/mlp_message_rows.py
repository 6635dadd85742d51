"""fp32 against 16-bit MLP-MP message rows (ptgnn_amd/precision.py `half_messages(mlp=True)`; csrc/gather_reduce16_epi.hip
and the row-storing per-edge GEMM with a target-state half of csrc/edge_gemm16.hip) in one process, bf16.

Two shapes: the cfg2 layer (benchmarks/synthetic.py make_cfg2: table form with a destination term, N = 200 k, E = 1.1 M,
H = M = 128, T = 1, sum) and a cfg4-like edge-form layer (benchmarks/mlp_inputs.py make_edge_layer at hidden 128:
E = 200 k, T = 21, max).  Per shape: the aggregation launch alone -- the fp32 kernel with destination term / epilogue on
fp32 rows against the new kernel on 16-bit rows -- and the producer launch alone (16-bit GEMM storing fp32 against 16-bit
rows), interleaved, three repeats of `--steps` launches, one HIP-event bracket per repeat, medians, next to the HBM
floors of their algorithmic bytes at 8 TB/s; then the layer inference forward under (a) fp32, (b) `mlp=True` alone (the
parent commit's route) and (c) `mlp=True` with the switch.  The record behind profiles/mlp_message_rows_notes.md:

    python -m benchmarks.mlp_message_rows [--out profiles/mlp_message_rows_bench.json] [--steps 10]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from benchmarks.edge_inputs import DEV, HBM_BYTES_PER_S, interleaved
from benchmarks.mlp_inputs import make_edge_layer, step
from ptgnn_amd import ops

BF16 = torch.bfloat16
SETTINGS = (("fp32", torch.float32, False), ("mlp_inputs", BF16, False), ("mlp_inputs_rows16", BF16, True))


def _floor_ms(nbytes):
    return round(nbytes / HBM_BYTES_PER_S * 1e3, 5)


def launches_alone(st, steps):
    """The layer's own aggregation and producer launches at the shape of `st`, fp32 rows against 16-bit rows."""
    from ptgnn_amd import layers as L
    layer, x, adj = st["layer"], st["x"], st["adj"]
    N, E, H, T = st["N"], st["E"], st["H"], len(adj)
    M, reduce = H, layer.export_weights()["agg"]
    plan = ops.plan_for(adj, N)
    edge_form = L._prefer_edge_path(E, N, T, H, M)
    epi = layer._epilogue(M, 512, cap_without_ln=False)
    res = {"form": "edge" if edge_form else "table", "reduce": reduce,
           "rows16_supported": ops.mlp_message_rows16_supported(x, M, BF16, H, T, edge_form, True)}
    with torch.no_grad():
        if edge_form:
            ws = [w.detach() for w in layer._first_weights()]
            kw = {"inputs": BF16, "rounded": torch.stack(ws).to(BF16).contiguous()}
            m32, m16 = ops.edge_linear(x, adj, ws, True, **kw), ops.edge_linear(x, adj, ws, True, rows=BF16, **kw)
            akw = dict(type_bits=0, col=plan.perm, **epi)
            fns = {"producer_rows32": lambda: ops.edge_linear(x, adj, ws, True, **kw),
                   "producer_rows16": lambda: ops.edge_linear(x, adj, ws, True, rows=BF16, **kw),
                   "aggregation_rows32": lambda: ops.gather_reduce(m32, plan, M, reduce, **akw),
                   "aggregation_rows16": lambda: ops.gather_reduce(m16, plan, M, reduce, **akw)}
            gemm = E * 8 * H + 4 * T * M * H + 16 * E
            floors = {"producer_rows32": gemm + E * 4 * M, "producer_rows16": gemm + E * 2 * M,
                      "aggregation_rows32": E * (4 * M + 4) + N * (4 * M + 4),
                      "aggregation_rows16": E * (2 * M + 4) + N * (4 * M + 4)}
        else:
            w = layer._stacked_edge_weights()
            w16 = w.to(BF16).contiguous()
            y32 = ops.linear(x, w, inputs=BF16, rounded=w16)
            y16 = ops.linear(x, w, inputs=BF16, rounded=w16, rows=BF16)
            (s32, d32), (s16, d16) = layer._table_halves(y32, T), layer._table_halves(y16, T)
            fns = {"producer_rows32": lambda: ops.linear(x, w, inputs=BF16, rounded=w16),
                   "producer_rows16": lambda: ops.linear(x, w, inputs=BF16, rounded=w16, rows=BF16),
                   "aggregation_rows32": lambda: ops.gather_reduce(s32, plan, M, reduce, ydst=d32, **epi),
                   "aggregation_rows16": lambda: ops.gather_reduce(s16, plan, M, reduce, ydst=d16, **epi)}
            n_out = w.shape[0]
            floors = {"producer_rows32": N * (4 * H + 4 * n_out) + 2 * n_out * H,
                      "producer_rows16": N * (4 * H + 2 * n_out) + 2 * n_out * H,
                      "aggregation_rows32": E * (4 * M + 4) + N * (4 * M + 4) + N * 4 * T * M,
                      "aggregation_rows16": E * (2 * M + 4) + N * (4 * M + 4) + N * 2 * T * M}
        res["launches"] = interleaved(fns, steps)
    med = {k: v["median_ms"] for k, v in res["launches"].items()}
    res["hbm_floor_ms"] = {k: _floor_ms(v) for k, v in floors.items()}
    res["over_hbm_floor"] = {k: round(med[k] / res["hbm_floor_ms"][k], 3) for k in med}
    res["ratios"] = {f"{k}_rows16_over_rows32": round(med[f"{k}_rows16"] / med[f"{k}_rows32"], 4)
                     for k in ("producer", "aggregation")}
    return res


def forward_settings(step_fn, steps, repeats=3):
    """Wall time per layer forward and per-kernel HIP-event times under the three settings, interleaved."""
    def under(dt, rows):
        return ptgnn_amd.matrix_inputs(dt, mlp=True), ptgnn_amd.half_messages(rows, mlp=rows)
    for _, dt, rows in SETTINGS:                      # warm-up: every setting, plan caches, allocator
        a, b = under(dt, rows)
        with a, b:
            for _ in range(2):
                step_fn()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _, _ in SETTINGS}
    for _ in range(repeats):
        for name, dt, rows in SETTINGS:
            a, b = under(dt, rows)
            with a, b:
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
    med = {k: v["ms_per_step_median"] for k, v in out.items()}
    out["rows16_over_mlp_inputs"] = round(med["mlp_inputs_rows16"] / med["mlp_inputs"], 4)
    out["rows16_over_fp32"] = round(med["mlp_inputs_rows16"] / med["fp32"], 4)
    return out


def main(out=None, steps=10):
    from benchmarks import synthetic
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16",
           "timing": f"3 interleaved repeats of {steps} launches (kernels) / steps (forward) per mode, medians",
           "baseline": "mlp_inputs / rows32 = the same process without the switch (the parent commit's launches)"}
    st = synthetic.make_cfg2(DEV, 0, 1)
    res["cfg2"] = {"workload": st["desc"], "alone": launches_alone(st, steps),
                   "layer_forward": forward_settings(lambda: synthetic.step_cfg2(st, 1), steps)}
    del st
    torch.cuda.empty_cache()
    st = make_edge_layer(hidden=128)
    res["cfg4_like"] = {"workload": st["desc"], "alone": launches_alone(st, steps),
                        "layer_forward": forward_settings(lambda: step(st), steps)}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/mlp_message_rows_bench.json")
    parser.add_argument("--steps", type=int, default=10)
    args = parser.parse_args()
    main(args.out, args.steps)
