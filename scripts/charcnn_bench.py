#!/usr/bin/env python
"""Timings behind profiles/charcnn_notes.md: the char-CNN embedder at N strings x 15 chars, 70 characters, the reference's
default CnnConfig(256, 3, 128, 3, 3), embedding size 128.

    python scripts/charcnn_bench.py [--n 116000] [--out profiles/charcnn_bench.json]

HIP events around one call, 10 warm-up calls, 50 timed calls, median (min / p90 kept).  Both routes run in one process on the
same tensors: "composed" is what the operators before the char-CNN kernels can do (window ids through the embedding bag,
windows copied in front of `dense.linear`).  The windowed GEMMs are timed next to `ops.linear` at the same k and n on
contiguous rows, as fractions of the 157 TFLOP/s fp32-MFMA peak.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptgnn_amd import embeddings, ops  # noqa: E402

PEAK = 157e12
DEV = torch.device("cuda")


def timed(fn, warmup=10, iters=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    times.sort()
    return {"median_us": statistics.median(times), "min_us": times[0], "p90_us": times[int(0.9 * len(times))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=116000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, L, C, D = args.n, 15, 70, 128
    cfg = embeddings.CnnConfig(256, 3, 128, 3, 3)
    k1, k2, k3, F1, F2 = cfg.l1_window_size, cfg.l2_window_size, cfg.lout_window_size, cfg.l1_filters, cfg.l2_filters
    R = L - k1 + 1
    rows = N * R
    torch.manual_seed(0)
    module = embeddings.CharUnitEmbedder(C, D, cfg).to(DEV)
    gen = torch.Generator().manual_seed(1)
    chars = torch.randint(1, C, (N, L), generator=gen)
    lengths = torch.randint(1, L + 1, (N,), generator=gen)
    chars[torch.arange(L).unsqueeze(0) >= lengths.unsqueeze(1)] = 0          # padded like CharTensorizer
    chars = chars.to(DEV)
    coef = torch.randn(N, D, device=DEV)
    result = {"shape": {"N": N, "L": L, "C": C, "config": list(cfg), "D": D, "rows": rows}}

    # ---- 1. the char-embed pieces against the composed bag route ----
    w1 = module._CharUnitEmbedder__conv_l1.weight.detach()
    b1 = module._CharUnitEmbedder__conv_l1.bias.detach()
    table = w1.permute(2, 1, 0).reshape(k1 * C, F1).contiguous()
    a1 = ops.char_embed(chars, table, b1, k1)
    g1 = torch.randn(rows, F1, device=DEV)

    def composed_embed(tab, bias):
        ids = (chars.clamp(0, C - 1).unfold(1, k1, 1) + torch.arange(k1, device=DEV) * C).reshape(rows, k1)
        lens = torch.full((rows,), k1, dtype=torch.int64, device=DEV)
        return torch.relu(embeddings.embedding_bag(tab, ids, lens, "sum") + bias)

    def composed_embed_train():
        tab, bias = table.clone().requires_grad_(True), b1.clone().requires_grad_(True)
        composed_embed(tab, bias).backward(g1)
        return tab.grad, bias.grad

    def fused_embed_train():
        out = ops.char_embed(chars, table, b1, k1)
        return ops.char_embed_backward(g1, out, chars, C, k1)

    fused_grads, composed_grads = fused_embed_train(), composed_embed_train()
    result["char_embed"] = {
        "forward_fused": timed(lambda: ops.char_embed(chars, table, b1, k1)),
        "forward_composed": timed(lambda: composed_embed(table, b1)),
        "backward_fused": timed(lambda: ops.char_embed_backward(g1, a1, chars, C, k1)),
        "forward_backward_fused": timed(fused_embed_train),
        "forward_backward_composed": timed(composed_embed_train),
        "max_abs_diff_forward": float((composed_embed(table, b1) - a1).abs().max()),
        "max_rel_diff_table_grad": float((fused_grads[0] - composed_grads[0]).abs().max() / composed_grads[0].abs().max()),
    }
    del g1, fused_grads, composed_grads

    # ---- 2. the windowed GEMMs next to ops.linear on contiguous rows ----
    gemms = {}
    for name, c_in, w, n_out in (("conv2", F1, k2, F2), ("conv3", F2, k3, D)):
        frame = torch.randn(rows + w - 1, c_in, device=DEV)
        weight = torch.randn(n_out, w * c_in, device=DEV) * 0.05
        dense_x = frame.unfold(0, w, 1).permute(0, 2, 1).reshape(rows, w * c_in).contiguous()
        flops = 2.0 * rows * w * c_in * n_out
        before = ops.launch_counts()
        yw = ops.window_linear(frame, 0, rows, w, weight)
        kernels = ops.launches_since(before)
        yd = ops.linear(dense_x, weight)
        tw, td = timed(lambda: ops.window_linear(frame, 0, rows, w, weight)), timed(lambda: ops.linear(dense_x, weight))
        g = torch.randn(rows, n_out, device=DEV)
        before = ops.launch_counts()
        gw = ops.window_weight_grad(frame, 0, rows, w, g)
        wkernels = ops.launches_since(before)
        gd = ops.linear_weight_grad(dense_x, g)
        tgw = timed(lambda: ops.window_weight_grad(frame, 0, rows, w, g))
        tgd = timed(lambda: ops.linear_weight_grad(dense_x, g))
        gemms[name] = {
            "k": w * c_in, "n": n_out, "flops": flops, "kernels": kernels, "weight_grad_kernels": wkernels,
            "windowed": tw, "contiguous": td, "same_bits": bool(torch.equal(yw, yd)),
            "windowed_fraction_of_peak": flops / (tw["median_us"] * 1e-6) / PEAK,
            "contiguous_fraction_of_peak": flops / (td["median_us"] * 1e-6) / PEAK,
            "weight_grad_windowed": tgw, "weight_grad_contiguous": tgd, "weight_grad_same_bits": bool(torch.equal(gw, gd)),
            "weight_grad_windowed_fraction_of_peak": flops / (tgw["median_us"] * 1e-6) / PEAK,
            "weight_grad_contiguous_fraction_of_peak": flops / (tgd["median_us"] * 1e-6) / PEAK,
        }
        del frame, dense_x, yw, yd, g, gw, gd
    result["gemm"] = gemms
    torch.cuda.empty_cache()

    # ---- 3. the whole module, windowed against composed ----
    def forward():
        with torch.no_grad():
            return module(chars)

    def train():
        module.zero_grad(set_to_none=True)
        (module(chars) * coef).sum().backward()

    before = ops.launch_counts(aggregation=True, char_cnn=True)
    train()
    result["module_kernels_windowed"] = ops.launches_since(before)
    out_w = forward()
    mod = {"forward_windowed": timed(forward), "forward_backward_windowed": timed(train)}
    grads_w = [p.grad.clone() for p in module.parameters()]
    supported = ops.char_embed_supported
    ops.char_embed_supported = lambda *a: False                      # the composed route of the same module
    try:
        before = ops.launch_counts(aggregation=True, char_cnn=True)
        train()
        result["module_kernels_composed"] = ops.launches_since(before)
        out_c = forward()
        mod["forward_composed"], mod["forward_backward_composed"] = timed(forward), timed(train)
        grads_c = [p.grad.clone() for p in module.parameters()]
    finally:
        ops.char_embed_supported = supported
    mod["max_abs_diff_forward"] = float((out_w - out_c).abs().max())
    mod["max_rel_diff_grads"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads_w, grads_c))
    mod["peak_memory_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    result["module"] = mod

    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
