"""EGCMessagePassingLayer timings on the cfg3 Graph2Class batch (48 graphs, ~116 k nodes, T = 17 after backward and
self edges, ~625 k edges), H = D = 128, K = 8 heads, B = 4 bases, max aggregation.  Not part of bench.py.

    python scripts/egc_bench.py [--out FILE] [--reps N]

Reports (HIP events, median of --reps, after warm-up):
  * layer inference and training step (forward + backward) against a torch restatement of the reference sequence
    (index_select, torch Linear, cat, ptgnn_amd.scatter.scatter, mul, sum) on the same GPU;
  * the fused aggregate + combine launch against plain gather_reduce at msg_dim 512 on the same plan and messages;
  * egc_combine_backward's algorithmic bandwidth (read agg, g, w; write g_agg, g_w).
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/egc_bench.py` run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import layers as L, ops, scatter, workloads  # noqa: E402


def t_med(fn, reps):
    for _ in range(3):
        fn()
    evs = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def torch_egc(x, adj, bases, wc, K, B, D, agg):
    """egcmessagepassing.py:63-91 with torch operators (the reference's sequence on the GPU)."""
    w = torch.nn.functional.linear(x, wc.weight, wc.bias).reshape(-1, K, B, 1)
    msgs = [torch.nn.functional.linear(x.index_select(0, s), lin.weight).reshape(-1, K, B, D // K)
            for (s, _), lin in zip(adj, bases)]
    m = torch.cat(msgs, dim=0)
    a = scatter.scatter(m.reshape(m.shape[0], -1), torch.cat([d for _, d in adj]), dim=0, dim_size=x.shape[0],
                        reduce=agg).reshape(-1, K, B, D // K)
    return (a * w).sum(axis=-2).reshape(-1, D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    dev = torch.device("cuda")
    H = D = 128
    K, B, agg = 8, 4, "max"
    mb = workloads.batched_graphs(48, 2500, 8, 2.2, seed=1234)
    N = mb["num_nodes"]
    ident = torch.arange(N)
    adj = list(mb["adjacency_lists"]) + [(d, s) for s, d in mb["adjacency_lists"]] + [(ident, ident)]
    adj = [(s.to(dev), d.to(dev)) for s, d in adj]
    T, E = len(adj), sum(int(s.shape[0]) for s, _ in adj)
    torch.manual_seed(1)
    layer = L.EGCMessagePassingLayer(H, D, T, agg, num_bases=B, num_heads=K).to(dev)
    x = workloads.node_states(N, H, seed=5).to(dev)
    feats = [torch.empty(s.shape[0], 0, device=dev) for s, _ in adj]
    gout = torch.randn(N, D, device=dev)
    res = {"N": N, "E": E, "T": T, "H": H, "D": D, "K": K, "B": B, "agg": agg, "reps": args.reps}

    layer.eval()
    with torch.no_grad():
        got = layer(x, adj, None, {}, {}, feats)
        want = torch_egc(x, adj, layer._EGCMessagePassingLayer__bases, layer._EGCMessagePassingLayer__weight_coeffs,
                         K, B, D, agg)
        res["max_abs_vs_torch"] = float((got - want).abs().max())
        res["infer_ms"] = t_med(lambda: layer(x, adj, None, {}, {}, feats), args.reps)
        res["infer_torch_ms"] = t_med(lambda: torch_egc(x, adj, layer._EGCMessagePassingLayer__bases,
                                                        layer._EGCMessagePassingLayer__weight_coeffs, K, B, D, agg),
                                      args.reps)
    layer.train()
    xg = x.clone().requires_grad_(True)

    def step_ours():
        layer.zero_grad(set_to_none=True)
        layer(xg, adj, None, {}, {}, feats).backward(gout)

    def step_torch():
        layer.zero_grad(set_to_none=True)
        torch_egc(xg, adj, layer._EGCMessagePassingLayer__bases, layer._EGCMessagePassingLayer__weight_coeffs,
                  K, B, D, agg).backward(gout)

    res["train_step_ms"] = t_med(step_ours, args.reps)
    res["train_step_torch_ms"] = t_med(step_torch, args.reps)
    res["infer_speedup"] = res["infer_torch_ms"] / res["infer_ms"]
    res["train_speedup"] = res["train_step_torch_ms"] / res["train_step_ms"]

    # fused aggregate + combine vs plain gather_reduce, same plan and messages (edge form: one message row per edge)
    with torch.no_grad():
        plan = ops.plan_for(adj, N)
        wc = layer._EGCMessagePassingLayer__weight_coeffs
        coef = ops.linear(x, wc.weight, wc.bias)
        msgs = ops.edge_linear(x, adj, [l.weight for l in layer._EGCMessagePassingLayer__bases], False)
        M = B * D
        res["gather_reduce_512_ms"] = t_med(
            lambda: ops.gather_reduce(msgs, plan, M, agg, type_bits=0, col=plan.perm), args.reps)
        res["egc_gather_combine_ms"] = t_med(
            lambda: ops.gather_combine(msgs, plan, K, B, D // K, agg, coef, type_bits=0, col=plan.perm), args.reps)
        res["fused_over_plain"] = res["egc_gather_combine_ms"] / res["gather_reduce_512_ms"]
        agg_t = ops.gather_reduce(msgs, plan, M, agg, type_bits=0, col=plan.perm)
        res["edge_linear_ms"] = t_med(
            lambda: ops.edge_linear(x, adj, [l.weight for l in layer._EGCMessagePassingLayer__bases], False),
            args.reps)
        res["egc_combine_ms"] = t_med(lambda: ops.basis_combine(agg_t, coef, K, B, D // K), args.reps)
        res["egc_combine_backward_ms"] = t_med(
            lambda: ops.basis_combine_backward(agg_t, coef, gout, K, B, D // K), args.reps)
        nbytes = 4.0 * N * (2 * B * D + D + 2 * K * B)     # read agg, g, w; write g_agg, g_w
        res["egc_combine_backward_bytes"] = nbytes
        res["egc_combine_backward_TBps"] = nbytes / (res["egc_combine_backward_ms"] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
