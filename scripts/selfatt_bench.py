"""MultiHeadSelfAttentionMessagePassing timings (selfattmessagepassing.py:9-136: D = 256, 8 heads, dk = dv = 32,
intermediate 1024, max_num_nodes = 250).  Not part of bench.py.

    python scripts/selfatt_bench.py [--out FILE] [--reps N]

The two batches of profiles/attnpool_notes.md: (a) 48 graphs / 107 k nodes; (b) 4 000 graphs / 114 k nodes.  Per batch
(HIP events, median of --reps after warm-up):
  * the fused attention (ops.block_attention) and its backward, with their share of the 157 TF fp32-MFMA peak on
    FLOP = sum over windows of heads * 2 n^2 (dk + dv) forward (3.5 x that backward: the scores and dP are recomputed
    in both gradient kernels);
  * module inference and a training step (forward + backward w.r.t. x and every weight) against a comparison route: the
    reference's forward line by line on torch's own operators on the same GPU (a Python loop of einsum / softmax / einsum
    per window, rocBLAS Linears) with autograd through the attention.  It is the baseline, never the code under test.
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/selfatt_bench.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import layers as L, ops  # noqa: E402

PEAK_TF = 157.3
D, H, DK, DV, INTER, MAXN = 256, 8, 32, 32, 1024, 250


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


def window_bounds(sizes):
    out, first = [], 0
    for c in sizes:
        out += [(first + lo, first + min(lo + MAXN, c)) for lo in range(0, c, MAXN)]
        first += c
    return out


def torch_reference(module, x, bounds):
    """selfattmessagepassing.py:92-123 on torch's operators (the windows precomputed on the host: the reference reads
    them back from the device once per forward)."""
    F = torch.nn.functional
    sd = {k.split("__")[-1]: v for k, v in module.named_parameters()}
    kqv = F.linear(x, sd["selfatt_head_transforms.weight"]).reshape(x.shape[0], H, -1)
    keys, queries, values = kqv[:, :, :DK], kqv[:, :, DK:2 * DK], kqv[:, :, 2 * DK:]
    outs = []
    for lo, hi in bounds:
        scores = torch.einsum("khd,vhd->khv", keys[lo:hi], queries[lo:hi]) / (DK ** 0.5)
        outs.append(torch.einsum("khv,vhd->khd", F.softmax(scores, dim=-1), values[lo:hi]))
    vals = torch.cat(outs, dim=0)
    out = F.linear(vals.reshape(vals.shape[0], -1), sd["summarization_layer.weight"])
    a = F.layer_norm(out + x, (D,), sd["layer_norm1.weight"], sd["layer_norm1.bias"])
    inter = F.relu(F.linear(a, sd["intermediate_layer.weight"], sd["intermediate_layer.bias"]))
    out = F.linear(inter, sd["output_layer.weight"], sd["output_layer.bias"])
    return F.layer_norm(out + a, (D,), sd["layer_norm2.weight"], sd["layer_norm2.bias"])


def run_batch(name, sizes, module, reps):
    g = torch.Generator().manual_seed(7)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).cuda()
    N = idx.shape[0]
    x = torch.randn(N, D, generator=g).cuda()
    bounds = window_bounds(sizes)
    flop = float(sum(H * 2 * (hi - lo) ** 2 * (DK + DV) for lo, hi in bounds))
    res = {"batch": name, "N": N, "G": len(sizes), "windows": len(bounds), "attention_flop": flop}
    with torch.no_grad():
        got, want = module(x, [], idx, {}, {}, []), torch_reference(module, x, bounds)
        res["max_abs_vs_torch"] = float((got - want).abs().max())
        plan = L._index_plan(idx, len(sizes))
        windows = ops.attention_windows(plan, MAXN)
        kqv = torch.randn(N, H * (2 * DK + DV), generator=g).cuda()
        out, lse = ops.block_attention(kqv, windows, MAXN, H, DK, DV)
        gout = torch.randn(N, H * DV, generator=g).cuda()
        res["windows_ms"] = t_med(lambda: ops.attention_windows(plan, MAXN), reps)
        res["attention_ms"] = t_med(lambda: ops.block_attention(kqv, windows, MAXN, H, DK, DV), reps)
        res["attention_tflops"] = flop / (res["attention_ms"] * 1e-3) / 1e12
        res["attention_frac_of_peak"] = res["attention_tflops"] / PEAK_TF
        res["attention_backward_ms"] = t_med(
            lambda: ops.block_attention_backward(kqv, out, lse, gout, windows, MAXN, H, DK, DV), reps)
        res["attention_backward_tflops"] = 3.5 * flop / (res["attention_backward_ms"] * 1e-3) / 1e12
        res["attention_backward_frac_of_peak"] = res["attention_backward_tflops"] / PEAK_TF
        res["infer_ms"] = t_med(lambda: module(x, [], idx, {}, {}, []), reps)
        res["infer_torch_ms"] = t_med(lambda: torch_reference(module, x, bounds), reps)
    xg = x.clone().requires_grad_(True)
    gy = torch.randn(N, D, generator=g).cuda()

    def step_ours():
        module.zero_grad(set_to_none=True)
        module(xg, [], idx, {}, {}, []).backward(gy)

    def step_torch():
        module.zero_grad(set_to_none=True)
        torch_reference(module, xg, bounds).backward(gy)

    res["train_step_ms"] = t_med(step_ours, reps)
    res["train_step_torch_ms"] = t_med(step_torch, reps)
    res["infer_speedup"] = res["infer_torch_ms"] / res["infer_ms"]
    res["train_speedup"] = res["train_step_torch_ms"] / res["train_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    torch.manual_seed(1)
    module = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, H, max_num_nodes=MAXN).cuda().eval()
    g = torch.Generator().manual_seed(3)
    big = (torch.rand(48, generator=g) * 1600 + 1620).long().tolist()       # ~107 k nodes in 48 graphs
    small = (torch.rand(4000, generator=g) * 30 + 14).long().tolist()       # ~114 k nodes in 4 000 graphs
    out = {"D": D, "heads": H, "dk": DK, "dv": DV, "intermediate": INTER, "max_num_nodes": MAXN, "reps": args.reps,
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
