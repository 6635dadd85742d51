"""The grouped per-edge GEMM of the GGNN edge form with fp32 against 16-bit matrix inputs (ptgnn_amd/precision.py,
`edge_gemm=True`; csrc/edge_gemm16.hip) in one process, at the cfg3 layer shapes.  The arguments of the layer's own
launch are captured from one cfg3 forward (node states, the 17 adjacency lists, the plan's unique-row table, the
weights), then the fp32 and the 16-bit launches of both forms run interleaved on them: three repeats of `--steps`
launches per mode, one HIP-event bracket per repeat, medians.  From the unique-row count, the HBM floor of the 16-bit
launch: rows (H + M) 4 bytes plus the 16-bit weights, at 8 TB/s.  Then the cfg3 forward under
`matrix_inputs(bfloat16)` with and without `edge_gemm=True`, next to fp32, the same way as benchmarks/half_inputs.py.
The record behind profiles/edge_inputs_notes.md:

    python -m benchmarks.edge_inputs [--out profiles/edge_inputs_bench.json] [--steps 5]
"""
import argparse
import json
import os
import statistics
import time

import torch

import ptgnn_amd
from ptgnn_amd import ops

DEV = torch.device("cuda")
HBM_BYTES_PER_S = 8e12
FORWARD_MODES = (("float32", torch.float32, False), ("bfloat16", torch.bfloat16, False),
                 ("bfloat16_edge_gemm", torch.bfloat16, True))
# developer A/B knobs of csrc/edge_gemm16.hip, read per launch: the workgroups per CU of the weight-stationary kernel (the
# default is what a CU holds at once: one resident round), and the per-wave kernel in its place
VARIANTS = (("one_resident_round", {}),) \
    + tuple((f"ws_{n}_per_cu", {"PTGNN_AMD_EDGE16_WGS": str(n)}) for n in (2, 3, 4, 6, 8, 12)) \
    + (("per_wave", {"PTGNN_AMD_EDGE16_WS": "0"}),)


def capture_edge_calls(st, step):
    """[(node states, adjacency lists, plan, weights)] of every `_edge_messages` call of one forward."""
    from ptgnn_amd import layers as L
    calls, real = [], L._edge_messages

    def spy(table, adjacency_lists, plan, weights, **kw):
        calls.append((table.detach().clone(), adjacency_lists, plan, [w.detach() for w in weights]))
        return real(table, adjacency_lists, plan, weights, **kw)
    L._edge_messages = spy
    try:
        step()
    finally:
        L._edge_messages = real
    torch.cuda.synchronize()
    return calls


def interleaved(fns, steps, repeats=3):
    """{name: median over `repeats` of the HIP-event time per launch of `steps` back-to-back launches}, the modes
    interleaved inside every repeat."""
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
    return {name: {"ms_per_launch": v, "median_ms": statistics.median(v)} for name, v in ms.items()}


def with_env(env, fn):
    def run():
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return run


def kernel_alone(call, steps):
    x, adj, plan, ws = call
    T, (M, H) = len(ws), ws[0].shape
    uq = plan.unique_messages()
    if uq is None:
        return {"shape": f"H={H} M={M} T={T}", "skipped": "the plan has no unique-row table (back-off)"}
    rows, E = int(uq.rows(wait=True)), plan.num_edges
    res = {"shape": f"H={H} M={M} T={T}", "nodes": int(x.shape[0]), "edges": E, "unique_rows": rows,
           "unique_rows_per_type": uq.host_counts(wait=True)[:-1],
           "hbm_floor_ms_16bit_shared": round((rows * (H + M) * 4 + T * M * H * 2) / HBM_BYTES_PER_S * 1e3, 5),
           "hbm_floor_ms_16bit_per_edge": round((E * (H + M) * 4 + T * M * H * 2) / HBM_BYTES_PER_S * 1e3, 5),
           "mfma_floor_note": "2 rows H M FLOP: fp32 MFMA 157 TFLOP/s, 16-bit MFMA 2.5 PFLOP/s (dense peaks)",
           "fp32_mfma_floor_ms_shared": round(2.0 * rows * H * M / 157e12 * 1e3, 5)}
    stacks = {dt: torch.stack([w.to(dt) for w in ws]).contiguous() for dt in (torch.bfloat16, torch.float16)}
    with torch.no_grad():
        fns = {"shared_float32": lambda: ops.edge_linear_shared(x, uq, ws),
               "shared_bfloat16": lambda: ops.edge_linear_shared(x, uq, ws, inputs=torch.bfloat16,
                                                                 rounded=stacks[torch.bfloat16]),
               "shared_float16": lambda: ops.edge_linear_shared(x, uq, ws, inputs=torch.float16,
                                                                rounded=stacks[torch.float16]),
               "per_edge_float32": lambda: ops.edge_linear(x, adj, ws, False),
               "per_edge_bfloat16": lambda: ops.edge_linear(x, adj, ws, False, inputs=torch.bfloat16,
                                                            rounded=stacks[torch.bfloat16])}
        res["launches"] = interleaved(fns, steps)
        shared16 = fns["shared_bfloat16"]
        res["variants_shared_bfloat16"] = interleaved(
            {"shared_float32": fns["shared_float32"], **{name: with_env(env, shared16) for name, env in VARIANTS}}, steps)
    med = {k: v["median_ms"] for k, v in res["launches"].items()}
    res["shared_bf16_over_fp32"] = round(med["shared_bfloat16"] / med["shared_float32"], 4)
    res["per_edge_bf16_over_fp32"] = round(med["per_edge_bfloat16"] / med["per_edge_float32"], 4)
    res["shared_bf16_over_hbm_floor"] = round(med["shared_bfloat16"] / res["hbm_floor_ms_16bit_shared"], 3)
    return res


def forward_modes(step, steps, repeats=3):
    for _, dt, flag in FORWARD_MODES:                 # warm-up: every mode, plan caches, allocator
        with ptgnn_amd.matrix_inputs(dt, edge_gemm=flag):
            for _ in range(2):
                step()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}} for name, _, _ in FORWARD_MODES}
    for _ in range(repeats):
        for name, dt, flag in FORWARD_MODES:
            with ptgnn_amd.matrix_inputs(dt, edge_gemm=flag):
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


def main(out=None, steps=5):
    from benchmarks import graph2class as G2C
    res = {"device": torch.cuda.get_device_name(0),
           "timing": f"3 interleaved repeats of {steps} launches (kernels) / steps (forward) per mode, medians"}
    st = G2C.make_cfg3(DEV)
    calls = capture_edge_calls(st, lambda: G2C.step_cfg3(st))
    res["workload"] = st["desc"]
    res["edge_form_layers_per_forward"] = len(calls)
    shapes = {}
    for call in calls:                                # one record per distinct layer shape (7 x H = 128, 1 x H = 256)
        shapes.setdefault(tuple(call[3][0].shape), call)
    res["kernel_alone"] = [kernel_alone(call, steps) for call in shapes.values()]
    del calls, shapes
    torch.cuda.empty_cache()
    rec = forward_modes(lambda: G2C.step_cfg3(st), steps)
    f32 = rec["float32"]["ms_per_step_median"]
    res["cfg3_forward"] = {"modes": rec,
                           "bf16_over_fp32": round(rec["bfloat16"]["ms_per_step_median"] / f32, 4),
                           "bf16_edge_gemm_over_fp32": round(rec["bfloat16_edge_gemm"]["ms_per_step_median"] / f32, 4),
                           "bf16_edge_gemm_over_bf16": round(rec["bfloat16_edge_gemm"]["ms_per_step_median"]
                                                             / rec["bfloat16"]["ms_per_step_median"], 4)}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/edge_inputs_bench.json")
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    main(args.out, args.steps)
