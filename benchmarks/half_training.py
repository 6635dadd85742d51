"""GGNN training step (forward + backward of one layer) with fp32 against bf16 matrix inputs
(`ptgnn_amd.matrix_inputs(torch.bfloat16, training=True)`, ptgnn_amd/precision.py) in one process, at the cfg3 layer
shapes: the table form (N = 120 000 nodes of 48 graphs, H = M = 128, 3 edge types) and the GRU node alone at H = 128
and H = 256.  Per mode three repeats, interleaved (fp32, bf16, fp32, ...), after a warm-up of both; per-kernel HIP-event
times from `ops.KernelTimer`, wall time per step from a synchronised block.  Also the weight gradient alone at the
shapes those steps run it.  The yardstick is the fp32 kernels in the same process.  The record behind
profiles/half_training_notes.md:

    python -m benchmarks.half_training [--out profiles/half_training_bench.json] [--steps 5]
"""
import argparse
import json
import statistics
import time

import torch

import ptgnn_amd
from ptgnn_amd import dense, ops, precision

DEV = torch.device("cuda")
MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16))
# fp32 timer name -> its 16-bit counterpart
PAIRS = (("linear_weight_grad", "half_linear_weight_grad"), ("gru_cell", "half_gru_cell_train"),
         ("linear", "half_linear"))


def measure(step, steps, repeats=3):
    """{mode: {"ms_per_step": [per repeat], "kernels": {name: [avg ms per call, per repeat]}}}"""
    for _, dt in MODES:                              # warm-up: both modes, plan caches, allocator
        with ptgnn_amd.matrix_inputs(dt, training=True):
            for _ in range(2):
                step()
    torch.cuda.synchronize()
    out = {name: {"ms_per_step": [], "kernels": {}, "calls_per_step": {}} for name, _ in MODES}
    for _ in range(repeats):
        for name, dt in MODES:
            with ptgnn_amd.matrix_inputs(dt, training=True):
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
                    out[name]["calls_per_step"][k] = v["calls"] / steps
    for rec in out.values():
        rec["ms_per_step_median"] = statistics.median(rec["ms_per_step"])
        rec["ms_per_step_spread"] = round(max(rec["ms_per_step"]) - min(rec["ms_per_step"]), 4)
        rec["kernels_median_ms"] = {k: statistics.median(v) for k, v in rec["kernels"].items()}
        rec["kernels_spread_ms"] = {k: round(max(v) - min(v), 5) for k, v in rec["kernels"].items()}
        rec["kernel_ms_per_step"] = round(sum(rec["kernels_median_ms"][k] * rec["calls_per_step"][k]
                                              for k in rec["kernels_median_ms"]), 4)
    return out


def ratios(rec):
    f, b = rec["float32"]["kernels_median_ms"], rec["bfloat16"]["kernels_median_ms"]
    out = {"step": round(rec["bfloat16"]["ms_per_step_median"] / rec["float32"]["ms_per_step_median"], 4),
           "kernel_ms_per_step": round(rec["bfloat16"]["kernel_ms_per_step"] / rec["float32"]["kernel_ms_per_step"], 4)}
    for fp32, half in PAIRS:
        if fp32 in f and half in b:
            out[f"{half}_over_{fp32}"] = round(b[half] / f[fp32], 4)
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
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return round(statistics.median(ms), 5), round(ms[-1] - ms[0], 5)


def wgrad_alone(n, k, n_out):
    """The weight gradient alone: median and spread of 20 HIP-event brackets per mode (three rounds, interleaved), the
    HBM floor of reading both fp32 operands once at 8 TB/s, and the partial traffic of the 16-bit kernel."""
    g = torch.Generator().manual_seed(1)
    x, gy = torch.randn(n, k, generator=g).to(DEV), torch.randn(n, n_out, generator=g).to(DEV)
    chunk = ops.half_wgrad_chunk_rows(n, n_out, k)
    res = {"shape": f"rows={n} k={k} n_out={n_out}", "hbm_floor_ms": round(n * (k + n_out) * 4 / 8e12 * 1e3, 5),
           "chunk_rows": chunk, "partials": -(-n // chunk),
           "partial_bytes_over_operand_bytes": round(2.0 * -(-n // chunk) * (n_out * k + n_out) / (n * (k + n_out)), 4)}
    runs = {"float32": [], "bfloat16": []}
    for _ in range(3):
        runs["float32"].append(events(lambda: ops.linear_weight_grad(x, gy, want_bias=True)))
        runs["bfloat16"].append(events(lambda: ops.half_linear_weight_grad(x, gy, torch.bfloat16, want_bias=True)))
    for name, v in runs.items():
        res[f"ms_{name}"] = statistics.median(m for m, _ in v)
        res[f"ms_{name}_rounds"] = [m for m, _ in v]
    res["bf16_over_fp32"] = round(res["ms_bfloat16"] / res["ms_float32"], 4)
    return res


def linear_alone(n, k, n_out, add):
    """One forward / input-gradient GEMM alone, [n, k] x [k, n_out] (with `add`: plus the fp32 addend of the GRU's
    d_h launch): the timer above averages `linear` over shapes, this does not."""
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(n, k, generator=g).to(DEV), (torch.randn(n_out, k, generator=g) * 0.05).to(DEV)
    addend = torch.randn(n, n_out, generator=g).to(DEV) if add else None
    res = {"shape": f"rows={n} k={k} n_out={n_out} addend={add}"}
    for name, dt in MODES:
        w16 = w.to(dt) if dt is not torch.float32 else None
        fn = (lambda: ops.linear_add(x, w, addend, inputs=dt, rounded=w16)) if add else \
            (lambda: ops.linear(x, w, inputs=dt, rounded=w16))
        rounds = [events(fn)[0] for _ in range(3)]
        res[f"ms_{name}"], res[f"ms_{name}_rounds"] = statistics.median(rounds), rounds
    res["bf16_over_fp32"] = round(res["ms_bfloat16"] / res["ms_float32"], 4)
    return res


def main(out=None, steps=5):
    from ptgnn_amd import layers as L, workloads
    res = {"device": torch.cuda.get_device_name(0), "timing": f"3 interleaved repeats of {steps} steps per mode",
           "setting": "ptgnn_amd.matrix_inputs(torch.bfloat16, training=True) against the fp32 default"}

    H = 128
    for degree in (2.2, 4.4, 6.6, 8.8, 13.2):        # the cfg3 batch (degree 2.2, 17 types) takes the edge form: with
        mb = workloads.batched_graphs(48, 2500, 3, degree, seed=1234)       # 3 types, the first degree the table wins
        N, T = mb["num_nodes"], len(mb["adjacency_lists"])
        E = sum(int(s.shape[0]) for s, _ in mb["adjacency_lists"])
        if not L._prefer_edge_path(E, N, T, H, H):
            break
    adj = [(s.to(DEV), d.to(DEV)) for s, d in mb["adjacency_lists"]]
    x = workloads.node_states(N, H, seed=2).to(DEV).requires_grad_(True)
    torch.manual_seed(5)
    layer = L.GatedMessagePassingLayer(H, H, T, "sum").train().to(DEV)
    go = torch.randn(N, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    feats = [torch.empty(int(s.shape[0]), 0, device=DEV) for s, _ in adj]

    def layer_step():
        ops.clear_plan_cache()
        layer.zero_grad(set_to_none=True)
        x.grad = None
        with L.forward_scope():
            y = layer(x, adj, None, {}, {}, feats)
        y.backward(go)
    before = ops.launch_counts(half=True, half_training=True)
    with ptgnn_amd.matrix_inputs(torch.bfloat16, training=True):
        layer_step()
    families = ops.launches_since(before)
    rec = measure(layer_step, steps)
    res["layer_table_form"] = {"workload": f"one GGNN layer, table form: 48 graphs N={N} E={E} (degree {degree}) T={T} H=M={H}, sum, "
                                           f"forward + backward", "bf16_launches": families, "modes": rec,
                               "bf16_over_fp32": ratios(rec)}

    for hd in (128, 256):
        g = torch.Generator().manual_seed(hd)
        a = torch.randn(N, hd, generator=g).to(DEV).requires_grad_(True)
        h = torch.randn(N, hd, generator=g).to(DEV).requires_grad_(True)
        gru = torch.nn.GRUCell(hd, hd).to(DEV)
        gout = torch.randn(N, hd, generator=g).to(DEV)

        def gru_step():
            dense.clear_transposed_cache()
            gru.zero_grad(set_to_none=True)
            a.grad = h.grad = None
            dense.gru_cell(gru, a, h, inputs=precision.training_inputs(a)).backward(gout)
        rec = measure(gru_step, steps)
        res[f"gru_only_h{hd}"] = {"workload": f"GRU node alone: N={N} M=H={hd}, forward + backward", "modes": rec,
                                  "bf16_over_fp32": ratios(rec)}
        del a, h, gru, gout
        torch.cuda.empty_cache()

    res["weight_grad_alone"] = [wgrad_alone(N, 128, 384), wgrad_alone(N, 256, 768), wgrad_alone(N, 128, 128)]
    res["linear_alone"] = [linear_alone(N, 128, 384, False), linear_alone(N, 384, 128, False),
                           linear_alone(N, 384, 128, True), linear_alone(N, 768, 256, False),
                           linear_alone(N, 768, 256, True)]
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/half_training_bench.json")
    parser.add_argument("--steps", type=int, default=5)
    args = parser.parse_args()
    main(args.out, args.steps)
