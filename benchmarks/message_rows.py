"""fp32 against 16-bit GGNN message rows (ptgnn_amd/precision.py `half_messages`; csrc/gather_reduce16.hip and the
row-storing forms of csrc/edge_gemm16.hip, csrc/half_gemm.hip) in one process.  Edge form: the arguments of the layer's
own launches are captured from one cfg3 forward (benchmarks/edge_inputs.py), then the bf16 per-edge GEMM in both launch
forms and the aggregation run interleaved with fp32 and with 16-bit rows -- three repeats of `--steps` launches per
mode, one HIP-event bracket per repeat, medians -- next to the HBM floors of their byte counts at 8 TB/s: the GEMM
rows (4 H + 4 M) against rows (4 H + 2 M), the aggregation E (4 M + 4) + N (4 M + 4) against E (2 M + 4) + N (4 M + 4).
Then the cfg3 forward under `matrix_inputs(bfloat16, edge_gemm=True)` with and without the switch.  Table form: the same
at a cfg2-like shape (N = 200 k, E = 1.1 M, H = M = 128, one edge type, sum), one GGNN layer.  The baseline of every
ratio is the same process without the switch, which is what the parent commit runs.  The record behind
profiles/message_rows_notes.md:

    python -m benchmarks.message_rows [--out profiles/message_rows_bench.json] [--steps 5]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from benchmarks.edge_inputs import DEV, HBM_BYTES_PER_S, capture_edge_calls, interleaved
from ptgnn_amd import ops

BF16 = torch.bfloat16


def _floor_ms(nbytes):
    return round(nbytes / HBM_BYTES_PER_S * 1e3, 5)


def _ratios(launches, pairs):
    med = {k: v["median_ms"] for k, v in launches.items()}
    return {f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in pairs}


def edge_form_alone(call, reduce, steps):
    x, adj, plan, ws = call
    T, (M, H) = len(ws), ws[0].shape
    uq = plan.unique_messages()
    if uq is None:
        return {"shape": f"H={H} M={M} T={T}", "skipped": "the plan has no unique-row table (back-off)"}
    rows, E, N = int(uq.rows(wait=True)), plan.num_edges, int(x.shape[0])
    res = {"shape": f"H={H} M={M} T={T}", "nodes": N, "edges": E, "unique_rows": rows, "reduce": reduce,
           "rows16_supported": ops.message_rows16_supported(x, M, BF16),
           "hbm_floor_ms": {"gemm_shared_rows32": _floor_ms(rows * (4 * H + 4 * M) + 2 * T * M * H),
                            "gemm_shared_rows16": _floor_ms(rows * (4 * H + 2 * M) + 2 * T * M * H),
                            "gemm_per_edge_rows32": _floor_ms(E * (4 * H + 4 * M) + 2 * T * M * H),
                            "gemm_per_edge_rows16": _floor_ms(E * (4 * H + 2 * M) + 2 * T * M * H),
                            "aggregation_rows32": _floor_ms(E * (4 * M + 4) + N * (4 * M + 4)),
                            "aggregation_rows16": _floor_ms(E * (2 * M + 4) + N * (4 * M + 4))}}
    if not res["rows16_supported"]:
        return res
    stack = torch.stack([w.to(BF16) for w in ws]).contiguous()
    with torch.no_grad():
        kw = {"inputs": BF16, "rounded": stack}
        m32, m16 = ops.edge_linear_shared(x, uq, ws, **kw), ops.edge_linear_shared(x, uq, ws, rows=BF16, **kw)
        fns = {"gemm_shared_rows32": lambda: ops.edge_linear_shared(x, uq, ws, **kw),
               "gemm_shared_rows16": lambda: ops.edge_linear_shared(x, uq, ws, rows=BF16, **kw),
               "gemm_per_edge_rows32": lambda: ops.edge_linear(x, adj, ws, False, **kw),
               "gemm_per_edge_rows16": lambda: ops.edge_linear(x, adj, ws, False, rows=BF16, **kw),
               "aggregation_rows32": lambda: ops.gather_reduce(m32, plan, M, reduce, type_bits=0, col=uq.slot_row),
               "aggregation_rows16": lambda: ops.gather_reduce(m16, plan, M, reduce, type_bits=0, col=uq.slot_row)}
        res["launches"] = interleaved(fns, steps)
    res["ratios"] = _ratios(res["launches"], [(f"{k}_rows16", f"{k}_rows32")
                                              for k in ("gemm_shared", "gemm_per_edge", "aggregation")])
    res["over_hbm_floor"] = {k: round(v["median_ms"] / res["hbm_floor_ms"][k], 3) for k, v in res["launches"].items()}
    return res


def forward_modes(step, steps, setting, repeats=3):
    """{rows32, rows16}: wall time per forward and per-kernel HIP-event times under `setting`, the two interleaved."""
    modes = (("rows32", False), ("rows16", True))
    for _, on in modes:                               # warm-up: both modes, plan caches, allocator
        with ptgnn_amd.matrix_inputs(BF16, **setting), ptgnn_amd.half_messages(on):
            for _ in range(2):
                step()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _ in modes}
    for _ in range(repeats):
        for name, on in modes:
            with ptgnn_amd.matrix_inputs(BF16, **setting), ptgnn_amd.half_messages(on):
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
        rec["kernels_median_ms"] = {k: statistics.median(v) for k, v in rec.pop("kernels").items()}
    out["rows16_over_rows32"] = round(out["rows16"]["ms_per_step_median"] / out["rows32"]["ms_per_step_median"], 4)
    return out


def table_form(steps, n=200_000, edges=1_100_000, hidden=128, seed=2024):
    """One GGNN layer at the cfg2-like table shape: the [N, M] table Linear, the aggregation, the layer forward."""
    from ptgnn_amd import layers as L
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    layer = L.GatedMessagePassingLayer(hidden, hidden, 1, "sum").eval().to(DEV)
    x = torch.randn(n, hidden, generator=g).to(DEV)
    adj = [(torch.randint(0, n, (edges,), generator=g).to(DEV), torch.randint(0, n, (edges,), generator=g).to(DEV))]
    feats = [torch.empty(edges, 0, device=DEV)]
    plan = ops.plan_for(adj, n)
    w = layer.export_weights()["edge_w"][0].to(DEV)
    H = M = hidden
    res = {"shape": f"N={n} E={edges} H=M={hidden} T=1 sum", "table_form": not L._prefer_edge_path(edges, n, 1, H, M),
           "hbm_floor_ms": {"linear_rows32": _floor_ms(n * (4 * H + 4 * M) + 2 * M * H),
                            "linear_rows16": _floor_ms(n * (4 * H + 2 * M) + 2 * M * H),
                            "aggregation_rows32": _floor_ms(edges * (4 * M + 4) + n * (4 * M + 4)),
                            "aggregation_rows16": _floor_ms(edges * (2 * M + 4) + n * (4 * M + 4))}}
    with torch.no_grad():
        w16 = w.to(BF16).contiguous()
        y32, y16 = ops.linear(x, w, inputs=BF16, rounded=w16), ops.linear(x, w, inputs=BF16, rounded=w16, rows=BF16)
        fns = {"linear_rows32": lambda: ops.linear(x, w, inputs=BF16, rounded=w16),
               "linear_rows16": lambda: ops.linear(x, w, inputs=BF16, rounded=w16, rows=BF16),
               "aggregation_rows32": lambda: ops.gather_reduce(y32, plan, M, "sum"),
               "aggregation_rows16": lambda: ops.gather_reduce(y16, plan, M, "sum")}
        res["launches"] = interleaved(fns, steps)
        res["ratios"] = _ratios(res["launches"], [("linear_rows16", "linear_rows32"),
                                                  ("aggregation_rows16", "aggregation_rows32")])
        res["over_hbm_floor"] = {k: round(v["median_ms"] / res["hbm_floor_ms"][k], 3)
                                 for k, v in res["launches"].items()}
        res["layer_forward"] = forward_modes(lambda: layer(x, adj, None, {}, {}, feats), steps, {})
    return res


def main(out=None, steps=5):
    from benchmarks import graph2class as G2C
    res = {"device": torch.cuda.get_device_name(0),
           "timing": f"3 interleaved repeats of {steps} launches (kernels) / steps (forward) per mode, medians",
           "baseline": "rows32 = the same process without the switch (the parent commit's launches)"}
    st = G2C.make_cfg3(DEV)
    calls = capture_edge_calls(st, lambda: G2C.step_cfg3(st))
    res["workload"] = st["desc"]
    shapes = {}
    for call in calls:                                # one record per distinct layer shape
        shapes.setdefault(tuple(call[3][0].shape), call)
    res["edge_form_alone"] = [edge_form_alone(call, "max", steps) for call in shapes.values()]
    del calls, shapes
    torch.cuda.empty_cache()
    res["cfg3_forward"] = forward_modes(lambda: G2C.step_cfg3(st), steps, {"edge_gemm": True})
    del st
    torch.cuda.empty_cache()
    res["table_form"] = table_form(steps)
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/message_rows_bench.json")
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    main(args.out, args.steps)
