"""GGNN edge-form training step (forward + backward of one layer with per-edge dropout) with fp32 against bf16 matrix
inputs (`ptgnn_amd.matrix_inputs(torch.bfloat16, edge_training=True)`, ptgnn_amd/precision.py; the masked forms of
csrc/edge_gemm16.hip, csrc/edge_wgrad16.hip) in one process, at the cfg3 layer shapes: the Graph2Class synthetic batch
(node states, the 17 adjacency lists and the plan captured from one cfg3 forward), H = M = 128 and the 256-wide last
layer (H = 256, M = 128), dropout 0.1.  The three launches of the autograd node alone -- forward, input gradient, weight
gradient -- against their fp32 counterparts on the same mask bits, and the layer's forward + backward wall time: fp32 and
bf16 interleaved, three repeats after a warm-up of both, medians and spreads, with each launch's HBM floor at 8 TB/s.
The yardstick is the fp32 kernels in the same process.  The record behind profiles/edge_training_notes.md:

    python -m benchmarks.edge_training [--out profiles/edge_training_bench.json] [--steps 5]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from benchmarks.edge_inputs import capture_edge_calls
from ptgnn_amd import ops

DEV = torch.device("cuda")
HBM_BYTES_PER_S = 8e12
P, SEED = 0.1, 1234
MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))


def interleaved(fns, steps, repeats=3):
    """{name: per-launch HIP-event times of `steps` back-to-back launches, one per repeat; median, min, spread}, the
    modes interleaved inside every repeat, after a warm-up of all of them."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                fn()
            e.record()
            torch.cuda.synchronize()
            ms[name].append(round(s.elapsed_time(e) / steps, 5))
    return {name: {"ms_per_launch": v, "median_ms": statistics.median(v), "min_ms": min(v),
                   "spread_ms": round(max(v) - min(v), 5)} for name, v in ms.items()}


def floor_ms(nbytes):
    return round(nbytes / HBM_BYTES_PER_S * 1e3, 5)


def kernels_alone(call, steps):
    """The node's three launches on the layer's own arguments and ONE mask: fp32 (the masked fp32 entries where they take
    the shape, else the hash form) against bf16."""
    x, adj, plan, ws = call
    T, (M, H) = len(ws), ws[0].shape
    E = plan.num_edges
    g = torch.randn(E, M, generator=torch.Generator().manual_seed(7)).to(DEV)
    bits = ops.dropout_bitmask(E, H, P, SEED, DEV)
    ident = [(i, i) for i in plan.identity_index()]
    wt = [w.t().contiguous() for w in ws]
    w16 = torch.stack(ws).to(torch.bfloat16).contiguous()
    wt16 = torch.stack(wt).to(torch.bfloat16).contiguous()
    mask_bytes = E * H / 8.0
    res = {"shape": f"H={H} M={M} T={T}", "nodes": int(x.shape[0]), "edges": E, "dropout": P,
           "edges_per_type": [int(s.shape[0]) for s, _ in adj],
           "wgrad16_chunk_edges": ops.edge_wgrad16_chunk_edges(E, T, M, H),
           "hbm_floor_ms": {
               "forward": floor_ms(E * (H + M) * 4 + 8 * E + mask_bytes + T * M * H * 2),
               "input_gradient": floor_ms(E * (H + M) * 4 + 8 * E + mask_bytes + T * M * H * 2),
               "weight_gradient": floor_ms(E * (H + M) * 4 + 8 * E + mask_bytes + T * M * H * 4)},
           "hbm_floor_note": "fp32 operand rows read or written once, ids, mask bits, weights; a gathered row counted per edge"}
    bf = torch.bfloat16
    with torch.no_grad():
        before = ops.launch_counts(edge16_training=True)
        fns = {
            "forward_float32": lambda: ops.edge_linear(x, adj, ws, False, dropout=(1, P, SEED), mask_bits=bits),
            "forward_bfloat16": lambda: ops.edge_linear(x, adj, ws, False, dropout=(1, P, SEED), mask_bits=bits, inputs=bf,
                                                        rounded=w16),
            "input_gradient_float32": lambda: ops.edge_linear(g, ident, wt, False, dropout=(2, P, SEED), mask_bits=bits),
            "input_gradient_bfloat16": lambda: ops.edge_linear(g, ident, wt, False, dropout=(2, P, SEED), mask_bits=bits,
                                                               inputs=bf, rounded=wt16),
            "weight_gradient_float32": lambda: ops.edge_weight_grad(x, adj, g, False, P, SEED, mask_bits=bits),
            "weight_gradient_bfloat16": lambda: ops.edge_weight_grad(x, adj, g, False, P, SEED, mask_bits=bits, inputs=bf)}
        for fn in fns.values():
            fn()
        res["families_of_one_call_each"] = ops.launches_since(before)
        res["launches"] = interleaved(fns, steps)
    for what in ("forward", "input_gradient", "weight_gradient"):
        f, b = res["launches"][what + "_float32"], res["launches"][what + "_bfloat16"]
        res[what + "_bf16_over_fp32"] = round(b["median_ms"] / f["median_ms"], 4)
        res[what + "_bf16_median_below_fp32_min"] = bool(b["median_ms"] < f["min_ms"])
        res[what + "_bf16_over_hbm_floor"] = round(b["median_ms"] / res["hbm_floor_ms"][what], 3)
    return res


def layer_step_times(call, steps, repeats=3):
    """Forward + backward wall time of one GGNN layer in train() with dropout P on the captured batch, per mode."""
    from ptgnn_amd import layers as L
    x0, adj, _, ws = call
    T, (M, H) = len(ws), ws[0].shape
    torch.manual_seed(5)
    layer = L.GatedMessagePassingLayer(H, M, T, "sum", dropout_rate=P).train().to(DEV)
    x = x0.detach().clone().requires_grad_(True)
    go = torch.randn(x.shape[0], H, generator=torch.Generator().manual_seed(3)).to(DEV)
    feats = [torch.empty(int(s.shape[0]), 0, device=DEV) for s, _ in adj]

    def step():
        ops.clear_plan_cache()
        layer.zero_grad(set_to_none=True)
        x.grad = None
        with L.forward_scope():
            y = layer(x, adj, None, {}, {}, feats)
        y.backward(go)
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _ in MODES}
    families = {}
    for name, dt in MODES:                              # warm-up: both modes, plan caches, allocator
        with ptgnn_amd.matrix_inputs(dt, edge_training=True):
            before = ops.launch_counts(half=True, edge16=True, half_training=True, edge16_training=True)
            step()
            families[name] = ops.launches_since(before)
            step()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, dt in MODES:
            with ptgnn_amd.matrix_inputs(dt, edge_training=True):
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
        rec["ms_per_step_min"] = min(rec["ms_per_step"])
        rec["ms_per_step_spread"] = round(max(rec["ms_per_step"]) - min(rec["ms_per_step"]), 4)
        rec["kernels_median_ms"] = {k: statistics.median(v) for k, v in rec["kernels"].items()}
    return {"workload": f"one GGNN layer, edge form, train(), dropout {P}: N={x.shape[0]} T={T} H={H} M={M}, sum, "
                        f"forward + backward", "launch_families_of_one_step": families, "modes": out,
            "bf16_over_fp32": round(out["bfloat16"]["ms_per_step_median"] / out["float32"]["ms_per_step_median"], 4),
            "bf16_median_below_fp32_min": bool(out["bfloat16"]["ms_per_step_median"] < out["float32"]["ms_per_step_min"])}


def main(out=None, steps=5):
    from benchmarks import graph2class as G2C
    res = {"device": torch.cuda.get_device_name(0),
           "timing": f"3 interleaved repeats of {steps} launches (kernels) / steps (layer) per mode, after a warm-up of both",
           "setting": "ptgnn_amd.matrix_inputs(torch.bfloat16, edge_training=True) against the fp32 default"}
    st = G2C.make_cfg3(DEV)
    calls = capture_edge_calls(st, lambda: G2C.step_cfg3(st))
    res["workload"] = st["desc"]
    shapes = {}
    for call in calls:                                # one record per distinct layer shape (7 x H = 128, 1 x H = 256)
        shapes.setdefault(tuple(call[3][0].shape), call)
    del calls, st
    torch.cuda.empty_cache()
    res["kernels_alone"] = [kernels_alone(call, steps) for call in shapes.values()]
    res["layer_step"] = [layer_step_times(call, steps) for call in shapes.values()]
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/edge_training_bench.json")
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    main(args.out, args.steps)
