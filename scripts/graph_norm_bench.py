"""GraphNorm timings (graphnorm.py:36-46) on the Graph2Class batch of benchmarks/graph2class.py (48 graphs, ~116 k nodes,
its own node_to_graph_idx) at D = 64 and D = 256, and on 4 000 small graphs of about 116 k nodes at D = 64 (the per-graph
folds and the serial fold of the parameter gradients over the graphs).  Not part of bench.py.

    python scripts/graph_norm_bench.py [--out FILE] [--reps N]

Per width (HIP events, median of --reps after warm-up, the two routes alternating):
  * forward under no_grad and forward + backward (w.r.t. x and the three parameters) of the fused route
    (layers.GraphNorm -> csrc/graph_norm.hip) against the composed route (layers._composed_graph_norm: the facade's HIP
    scatter_mean plus torch's elementwise operators, i.e. what running the reference class after
    `ptgnn_amd.scatter.install()` does);
  * the rate of both fused entry points on their algorithmic bytes -- forward 3 reads of x + 1 write of y, backward
    2 reads of (x, grad_y) + 1 write of grad_x, [N, D] fp32 each, plus the 4-byte plan entry per row and pass -- as a share
    of the 8 TB/s HBM peak (re-reads may be served by the Infinity Cache: the share is of HBM peak, not a claim that the
    bytes came from HBM).
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/graph_norm_bench.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import layers as L, ops, workloads  # noqa: E402

PEAK_TBPS = 8.0
WIDTHS = (64, 256)


def t_med_pair(fa, fb, reps):
    """Medians of two callables timed alternately (same call, same machine state)."""
    for _ in range(3):
        fa()
        fb()
    evs = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            evs[k].append((s, e))
    torch.cuda.synchronize()
    return tuple(sorted(a.elapsed_time(b) for a, b in ev)[reps // 2] for ev in evs)


def t_med(fn, reps):
    return t_med_pair(fn, lambda: None, reps)[0]


def run_width(name, D, idx, reps):
    N, G = idx.shape[0], int(idx.max()) + 1
    g = torch.Generator().manual_seed(100 + D)
    x = torch.randn(N, D, generator=g).cuda()
    gout = torch.randn(N, D, generator=g).cuda()
    layer = L.GraphNorm(D)
    with torch.no_grad():
        layer.gamma.copy_(0.5 + torch.rand(1, D, generator=g))
        layer.alpha.copy_(0.5 + torch.rand(1, D, generator=g))
        layer.bias.copy_(torch.randn(1, D, generator=g))
    layer = layer.cuda()
    eps = 1e-10
    res = {"batch": name, "D": D, "N": N, "G": G}

    def fused(inp):
        return layer(inp, [], idx, {}, {}, [])

    def composed(inp):
        return L._composed_graph_norm(inp, idx, G, layer.gamma, layer.alpha, layer.bias, eps)

    with torch.no_grad():
        res["max_abs_vs_composed"] = float((fused(x) - composed(x)).abs().max())
        res["forward_ms"], res["forward_composed_ms"] = t_med_pair(lambda: fused(x), lambda: composed(x), reps)
        plan = L._index_plan(idx, G)
        p = (layer.gamma, layer.alpha, layer.bias)
        _, mean = ops.graph_norm(x, *p, eps, plan, with_mean=True)
        fwd_bytes = 4.0 * 4 * N * D + 3 * 4.0 * N
        bwd_bytes = 4.0 * 5 * N * D + 2 * 4.0 * N
        res["entry_forward_ms"] = t_med(lambda: ops.graph_norm(x, *p, eps, plan, with_mean=True), reps)
        res["entry_backward_ms"] = t_med(lambda: ops.graph_norm_backward(x, gout, p[0], p[1], eps, mean, plan), reps)
        res["entry_forward_bytes"], res["entry_backward_bytes"] = fwd_bytes, bwd_bytes
        res["entry_forward_frac_of_hbm_peak"] = fwd_bytes / (res["entry_forward_ms"] * 1e-3) / 1e12 / PEAK_TBPS
        res["entry_backward_frac_of_hbm_peak"] = bwd_bytes / (res["entry_backward_ms"] * 1e-3) / 1e12 / PEAK_TBPS
    xg = x.clone().requires_grad_(True)

    def step(route):
        def run():
            layer.zero_grad(set_to_none=True)
            xg.grad = None
            route(xg).backward(gout)
        return run

    step(fused)()
    got = [xg.grad.clone()] + [q.grad.clone() for q in layer.parameters()]
    step(composed)()
    want = [xg.grad.clone()] + [q.grad.clone() for q in layer.parameters()]
    res["grad_max_rel_vs_composed"] = max(float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
                                          for a, b in zip(got, want))
    res["train_step_ms"], res["train_step_composed_ms"] = t_med_pair(step(fused), step(composed), reps)
    res["forward_speedup"] = res["forward_composed_ms"] / res["forward_ms"]
    res["train_speedup"] = res["train_step_composed_ms"] / res["train_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=31)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_norm_bench.py measures on the GPU; none is visible")
    idx = workloads.batched_graphs(48, 2500, 8, 2.2, seed=1234)["node_to_graph_idx"].cuda()
    g = torch.Generator().manual_seed(3)
    small = (torch.rand(4000, generator=g) * 30 + 14).long()                 # ~116 k nodes in 4 000 graphs
    idx_small = torch.repeat_interleave(torch.arange(4000), small).cuda()
    out = {"reps": args.reps,
           "widths": [run_width("graph2class_48", D, idx, args.reps) for D in WIDTHS]
           + [run_width("small_4000", 64, idx_small, args.reps)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
