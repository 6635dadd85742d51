"""MlpMessagePassingLayer + PnaMessageAggregation timings at the cfg2 shape (N = 200 k nodes, E = 1.1 M edges, one edge
type, H = M = 128, table form).  Not part of bench.py.

    python scripts/pna_bench.py [--out FILE] [--reps N]

Reports (HIP events, median of --reps, after warm-up):
  * the fused inference launch (aggregate, scalers, GELU, LayerNorm(15M)) and its algorithmic bandwidth
    E*(4M + 4) + N*(4M + 60M + 4) bytes (the table-form destination term included);
  * layer inference and a training step (forward + backward) against a torch restatement of the reference sequence
    (index_select, Linear, cat, index_add / scatter_reduce, pow, relu, sqrt, log, cat, GELU, LayerNorm, Linear, Tanh)
    on the same GPU;
  * pna_aggregate_backward's algorithmic bandwidth (read messages twice, A, args and dL/dout; write the message gradient).
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/pna_bench.py` run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import layers as L, ops  # noqa: E402


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


def torch_pna(m, t, n, delta):
    """pna_aggregation.py:27-56 with torch operators on the GPU."""
    M = m.shape[1]
    deg = torch.zeros(n, dtype=torch.int64, device=m.device).index_add_(0, t, torch.ones_like(t))
    idx = t.unsqueeze(1).expand(-1, M)
    s = torch.zeros(n, M, device=m.device).index_add(0, t, m)
    mean = s / (deg.unsqueeze(-1) + 1e-5)
    mx = torch.zeros(n, M, device=m.device).scatter_reduce(0, idx, m, "amax", include_self=False)
    mn = torch.zeros(n, M, device=m.device).scatter_reduce(0, idx, m, "amin", include_self=False)
    comp = torch.relu(m.pow(2) - mean[t].pow(2)) + 1e-10
    std = torch.sqrt(torch.zeros(n, M, device=m.device).index_add(0, t, comp))
    A = torch.cat([s, mean, mx, mn, std], dim=-1)
    s1 = torch.log(deg.float() + 1).unsqueeze(-1) / delta
    return torch.cat([A, A * s1, A * (1 / (s1 + 1e-3))], dim=-1)


def torch_layer(layer, x, adj):
    """mlpmessagepassing.py:80-117 with torch operators (single-Linear edge MLPs, target state as input)."""
    F = torch.nn.functional
    mlps = layer._MlpMessagePassingLayer__edge_message_transformation_layers
    msgs, tgts = [], []
    for (s, d), mlp in zip(adj, mlps):
        inp = torch.cat([x.index_select(0, s), x.index_select(0, d)], dim=-1)
        msgs.append(F.linear(inp, mlp.linears[0].weight))
        tgts.append(d)
    a = torch_pna(torch.cat(msgs), torch.cat(tgts), x.shape[0], layer._MlpMessagePassingLayer__aggregation_fn._delta)
    a = F.layer_norm(F.gelu(a), layer._ln.normalized_shape, layer._ln.weight, layer._ln.bias, layer._ln.eps)
    return torch.tanh(F.linear(a, layer._dense.weight, layer._dense.bias))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    dev = torch.device("cuda")
    N, E, H, M = 200_000, 1_100_000, 128, 128
    g = torch.Generator().manual_seed(1234)
    adj = [(torch.randint(0, N, (E,), generator=g).to(dev), torch.randint(0, N, (E,), generator=g).to(dev))]
    torch.manual_seed(1)
    layer = L.MlpMessagePassingLayer(H, H, M, 1, L.PnaMessageAggregation()).to(dev)
    x = torch.randn(N, H, generator=g).to(dev)
    feats = [torch.empty(E, 0, device=dev)]
    gout = torch.randn(N, H, device=dev)
    res = {"N": N, "E": E, "T": 1, "H": H, "M": M, "reps": args.reps}

    layer.eval()
    with torch.no_grad():
        got = layer(x, adj, None, {}, {}, feats)
        res["max_abs_vs_torch"] = float((got - torch_layer(layer, x, adj)).abs().max())
        res["infer_ms"] = t_med(lambda: layer(x, adj, None, {}, {}, feats), args.reps)
        res["infer_torch_ms"] = t_med(lambda: torch_layer(layer, x, adj), args.reps)
        plan = ops.plan_for(adj, N)
        y = ops.linear(x, layer._stacked_edge_weights())
        ln = layer._ln
        fused = dict(epilogue=ops.EPI_GELU_LAYERNORM, ln_weight=ln.weight, ln_bias=ln.bias, ln_eps=ln.eps)
        res["pna_aggregate_fused_ms"] = t_med(lambda: ops.pna_aggregate(y[:, :M], plan, M, ydst=y[:, M:], **fused),
                                              args.reps)
        nbytes = E * (4.0 * M + 4) + N * (4.0 * M + 60.0 * M + 4)
        res["pna_aggregate_fused_bytes"] = nbytes
        res["pna_aggregate_fused_TBps"] = nbytes / (res["pna_aggregate_fused_ms"] * 1e-3) / 1e12
        res["pna_aggregate_raw_ms"] = t_med(lambda: ops.pna_aggregate(y[:, :M], plan, M, ydst=y[:, M:]), args.reps)
        res["table_gemm_ms"] = t_med(lambda: ops.linear(x, layer._stacked_edge_weights()), args.reps)
        agg = ops.pna_aggregate(y[:, :M], plan, M, ydst=y[:, M:], **fused)
        res["dense_ms"] = t_med(lambda: ops.linear(agg, layer._dense.weight, layer._dense.bias, act="tanh"), args.reps)

        msgs = ops.edge_linear(x, adj, [layer._MlpMessagePassingLayer__edge_message_transformation_layers[0]
                                        .linears[0].weight], True)
        out, amax, amin = ops.pna_aggregate(msgs, plan, M, type_bits=0, col=plan.perm, return_arg=True)
        g15 = torch.randn(N, 15 * M, device=dev)
        res["pna_aggregate_backward_ms"] = t_med(
            lambda: ops.pna_aggregate_backward(msgs, plan, out, amax, amin, g15), args.reps)
        bbytes = E * (3 * 4.0 * M + 8) + N * (4.0 * (15 * M + 2 * M) + 8.0 * M + 4)
        res["pna_aggregate_backward_bytes"] = bbytes
        res["pna_aggregate_backward_TBps"] = bbytes / (res["pna_aggregate_backward_ms"] * 1e-3) / 1e12

    layer.train()
    xg = x.clone().requires_grad_(True)

    def step_ours():
        layer.zero_grad(set_to_none=True)
        layer(xg, adj, None, {}, {}, feats).backward(gout)

    def step_torch():
        layer.zero_grad(set_to_none=True)
        torch_layer(layer, xg, adj).backward(gout)

    res["train_step_ms"] = t_med(step_ours, args.reps)
    res["train_step_torch_ms"] = t_med(step_torch, args.reps)
    res["infer_speedup"] = res["infer_torch_ms"] / res["infer_ms"]
    res["train_speedup"] = res["train_step_torch_ms"] / res["train_step_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
