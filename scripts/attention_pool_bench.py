"""Graph2Seq node -> graph summariser timings (MultiheadSelfAttentionVarSizedElementReduce, graph2seq.py:116-122:
D = hidden = 256, 8 heads, `max` query, output 128).  Not part of bench.py.

    python scripts/attention_pool_bench.py [--out FILE] [--reps N]

Two batches of about 116 k elements: (a) the Graph2Class batch, 48 graphs; (b) 4 000 small graphs.  Per batch
(HIP events, median of --reps after warm-up):
  * the fused pool (ops.attention_pool) and its rate on the algorithmic bytes N*D*4 + G*heads*D*4 (+ u read, perm);
  * its backward (ops.attention_pool_backward) on 2*N*D*4 + 4*G*heads*D*4 (+ perm);
  * module inference and a training step (forward + backward w.r.t. x and every weight) against the reference's
    operator sequence (varsizedsummary.py:140-178) on the same GPU over the torch_scatter facade, i.e. what running the
    reference class after `ptgnn_amd.scatter.install()` does.
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/attention_pool_bench.py`."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import ops, reduceops as R, scatter as S  # noqa: E402

PEAK_TBPS = 8.0
D, H, OUT = 256, 8, 128


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


def facade_reference(module, x, idx, G):
    """varsizedsummary.py:140-178 line by line, torch_scatter = ptgnn_amd.scatter (HIP), Linears = torch."""
    F = torch.nn.functional
    sd = {k.split("__")[-1]: v for k, v in module.named_parameters()}
    queries = S.scatter(x, idx, dim=0, dim_size=G, reduce="max")
    qpe = queries[idx]
    qpe = qpe.reshape(qpe.shape[0], H, qpe.shape[1] // H)
    keys = F.linear(x, sd["key_layer.weight"])
    keys = keys.reshape(keys.shape[0], H, keys.shape[1] // H)
    scores = torch.einsum("bhk,bhk->bh", qpe, keys) / math.sqrt(keys.shape[-1])
    probs = torch.exp(S.scatter_log_softmax(scores, idx, dim=0, eps=0))
    outputs = (probs.unsqueeze(-1) * x.unsqueeze(1)).reshape(x.shape[0], -1)
    per_sample = S.scatter_sum(outputs, idx, dim=0, dim_size=G)
    return F.linear(per_sample, sd["output_layer.weight"])


def batch(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).cuda()
    return torch.randn(idx.shape[0], D, generator=g).cuda(), idx, len(sizes)


def run_batch(name, sizes, module, reps):
    x, idx, G = batch(sizes, 7)
    N = x.shape[0]
    res = {"batch": name, "N": N, "G": G}
    inp = R.ElementsToSummaryRepresentationInput(x, idx, G)
    with torch.no_grad():
        got, want = module(inp), facade_reference(module, x, idx, G)
        res["max_abs_vs_facade"] = float((got - want).abs().max())
        plan = R._index_plan(idx, G)
        q = R.SimpleVarSizedElementReduce("max")(inp)
        wk = module._MultiheadSelfAttentionVarSizedElementReduce__key_layer.weight
        u = ops.head_expand(q, wk, H, 1.0 / math.sqrt(D // H))
        pooled, stats = ops.attention_pool(x, u, plan)
        fwd_bytes = 4.0 * (N * D + 2 * G * H * D) + 4.0 * N
        res["pool_ms"] = t_med(lambda: ops.attention_pool(x, u, plan), reps)
        res["pool_bytes"] = fwd_bytes
        res["pool_frac_of_peak"] = fwd_bytes / (res["pool_ms"] * 1e-3) / 1e12 / PEAK_TBPS
        gP = torch.randn_like(pooled)
        bwd_bytes = 4.0 * (2 * N * D + 4 * G * H * D) + 4.0 * N
        res["pool_backward_ms"] = t_med(lambda: ops.attention_pool_backward(x, u, plan, pooled, stats, gP), reps)
        res["pool_backward_bytes"] = bwd_bytes
        res["pool_backward_frac_of_peak"] = bwd_bytes / (res["pool_backward_ms"] * 1e-3) / 1e12 / PEAK_TBPS
        res["head_expand_ms"] = t_med(lambda: ops.head_expand(q, wk, H, 1.0), reps)
        res["infer_ms"] = t_med(lambda: module(inp), reps)
        res["infer_facade_ms"] = t_med(lambda: facade_reference(module, x, idx, G), reps)
    xg = x.clone().requires_grad_(True)
    gout = torch.randn(G, OUT, device=x.device)
    ginp = R.ElementsToSummaryRepresentationInput(xg, idx, G)

    def step_ours():
        module.zero_grad(set_to_none=True)
        module(ginp).backward(gout)

    def step_facade():
        module.zero_grad(set_to_none=True)
        facade_reference(module, xg, idx, G).backward(gout)

    res["train_step_ms"] = t_med(step_ours, reps)
    res["train_step_facade_ms"] = t_med(step_facade, reps)
    res["infer_speedup"] = res["infer_facade_ms"] / res["infer_ms"]
    res["train_speedup"] = res["train_step_facade_ms"] / res["train_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    torch.manual_seed(1)
    module = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, OUT, H, R.SimpleVarSizedElementReduce("max")).cuda()
    g = torch.Generator().manual_seed(3)
    big = (torch.rand(48, generator=g) * 1600 + 1620).long().tolist()       # ~116 k nodes in 48 graphs
    small = (torch.rand(4000, generator=g) * 30 + 14).long().tolist()       # ~116 k nodes in 4 000 graphs
    out = {"D": D, "heads": H, "out": OUT, "reps": args.reps,
           "batches": [run_batch("graph2class_48", big, module, args.reps),
                       run_batch("small_4000", small, module, args.reps)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
