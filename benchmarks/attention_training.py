"""The attention layer's TRAINING step with fp32 against 16-bit matrix inputs (`ptgnn_amd.set_attention_training`;
csrc/block_attention16.hip with dropout, csrc/block_attention16_backward.hip) in one process, on the two batches and with
the timing method of benchmarks/attention_inputs.py: 48 graphs / ~107 k nodes and 4 000 graphs / ~114 k nodes, D = 256,
8 heads, dk = dv = 32, intermediate 1024, max_num_nodes 250; HIP events, median of 21 after warm-up.  The baseline is
the fp32 launches of the same run.

Per batch, dropout rate (0 and 0.1) and mode: the attention op's forward, its backward (row-dot + key-gradient +
query/value-gradient kernels) and their sum, and the layer's training step (forward + backward of a sum of squares).
The record behind profiles/attention_training_notes.md:

    python -m benchmarks.attention_training [--out profiles/attention_training_bench.json] [--reps 21]
"""
import argparse
import json

import torch

import ptgnn_amd
from benchmarks.attention_inputs import D, DEV, DK, DV, HEADS, INTER, MAXN, MODES, t_med, window_bounds
from ptgnn_amd import layers as L, ops

RATES = (0.0, 0.1)
SEED = 1234


def run_batch(name, sizes, reps):
    g = torch.Generator().manual_seed(7)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    n = idx.shape[0]
    x = torch.randn(n, D, generator=g).to(DEV)
    kqv = torch.randn(n, HEADS * (2 * DK + DV), generator=g).to(DEV)
    gout = torch.randn(n, HEADS * DV, generator=g).to(DEV)
    windows = ops.attention_windows(L._index_plan(idx, len(sizes)), MAXN)
    bounds = window_bounds(sizes)
    # forward 2 products, backward 5 (S and dP recomputed, dK, dQ, dV) per kernel pair
    flop = float(sum(HEADS * 2 * (hi - lo) ** 2 * (DK + DV) for lo, hi in bounds))
    res = {"batch": name, "N": n, "G": len(sizes), "windows": len(bounds), "forward_flop": flop, "rates": {}}
    for p in RATES:
        torch.manual_seed(1)
        module = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, dropout_rate=p,
                                                        max_num_nodes=MAXN).to(DEV).train()

        def step():
            module.zero_grad(set_to_none=True)
            module(x, [], idx, {}, {}, []).square().sum().backward()

        entry = {}
        for mode, dt in MODES:
            def forward():
                return ops.block_attention(kqv, windows, MAXN, HEADS, DK, DV, p, SEED, inputs=dt, masked16=True)

            out, lse = forward()

            def backward():
                return ops.block_attention_backward(kqv, out, lse, gout, windows, MAXN, HEADS, DK, DV, p, SEED, inputs=dt)

            before = ops.launch_counts(aggregation=True, attention16=True, attention16_training=True)
            forward(), backward()
            want = {"block_attention": 1, "block_attention_backward": 1} if dt == torch.float32 else \
                {"attention_train16" if p > 0 else "block_attention16": 1, "attention_train16_backward": 1}
            assert ops.launches_since(before) == want, ops.launches_since(before)
            fwd, bwd = t_med(forward, reps), t_med(backward, reps)
            with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training():
                entry[mode] = {"op_forward_ms": fwd, "op_backward_ms": bwd, "op_ms": fwd + bwd,
                               "layer_step_ms": t_med(step, reps)}
        for mode, _ in MODES[1:]:
            for key in ("op_forward_ms", "op_backward_ms", "op_ms", "layer_step_ms"):
                entry[mode][key.replace("_ms", "_over_float32")] = entry[mode][key] / entry["float32"][key]
        res["rates"][str(p)] = entry
    return res


def main(out=None, reps=21):
    g = torch.Generator().manual_seed(3)
    big = (torch.rand(48, generator=g) * 1600 + 1620).long().tolist()       # ~107 k nodes in 48 graphs
    small = (torch.rand(4000, generator=g) * 30 + 14).long().tolist()       # ~114 k nodes in 4 000 graphs
    res = {"device": torch.cuda.get_device_name(0), "D": D, "heads": HEADS, "dk": DK, "dv": DV, "intermediate": INTER,
           "max_num_nodes": MAXN, "timing": f"HIP events, median of {reps} after 3 warm-up calls",
           "batches": [run_batch("graph2class_48", big, reps), run_batch("small_4000", small, reps)]}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/attention_training_bench.json")
    parser.add_argument("--reps", type=int, default=21)
    args = parser.parse_args()
    main(args.out, args.reps)
