"""The decoder's score-free loss against its `fused_loss` (GruCopyingDecoder at the shapes of scripts/decoder_bench.py:
B = 64, L = 7, H = Dm = 128, E = 256, V = 20 000, 100 .. 500 memories per sample; dropout 0 and 0.2).  Not part of bench.py.

    python scripts/projection_loss_bench.py [--out FILE] [--window SECONDS] [--repeats N] [--kernels-only]
                                            [--dtype bfloat16|float16] [--dim E]

The protocol of scripts/graph2seq_bench.py: a training step of `score_free_loss` and of `fused_loss` on the SAME module in
the same process, alternating after a warm-up, each timed with device events over a window of at least --window seconds,
--repeats times; the peak of allocated memory above what was live before a step, after a collection.  Then the two entries
of csrc/projection_loss.hip alone (device events around the wrapper calls, median) against R V E multiply-adds per pass:
    projection_loss            1 pass   2 R V E flop    reads 4 V E ceil(R / 64) + 4 R E ceil(V / 256) bytes
    projection_loss_backward   4 passes 8 R V E flop    (two recomputations, two gradient products)
The times of the three kernels proper come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/projection_loss_bench.py --kernels-only`.

With --dtype the 16-bit-input route (csrc/projection_loss16.hip: `ptgnn_amd.vocabulary_loss()` under `matrix_inputs(dtype)`)
is a third party to every comparison, in the same process and the same alternation: its two entries beside the fp32 ones,
and its training step beside the fp32 `score_free_loss` and `fused_loss`.  --dim replaces the embedding width E."""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decoder_bench import B, DM, E, H, L, UNK, V, batch  # noqa: E402
from graph2seq_bench import median_ms, window_ms  # noqa: E402
import ptgnn_amd  # noqa: E402
from ptgnn_amd import ops, sequence  # noqa: E402

PEAK_FP32_MATRIX_TFLOPS = 157.3


def steps(dropout, window, repeats, dtype=None, E=E):
    torch.manual_seed(1)
    m = sequence.GruCopyingDecoder(V, E, H, DM, UNK, dropout).cuda().train()
    inp = batch(7)
    live = dict(inp, input_memories=inp["input_memories"].clone().requires_grad_(True),
                initial_states=inp["initial_states"].clone().requires_grad_(True))

    def step_of(fn):
        def step():
            m.zero_grad(set_to_none=True)
            fn(**live).backward()
        return step

    free, fused = step_of(m.score_free_loss), step_of(m.fused_loss)

    def free16():
        with ptgnn_amd.vocabulary_loss(), ptgnn_amd.matrix_inputs(dtype):
            free()
    res = {"dropout": dropout, "I": int(inp["input_memories"].shape[0]), "B": B, "L": L, "V": V, "E": E, "H": H}
    if dropout == 0.0:
        with torch.no_grad():
            res["loss_score_free"], res["loss_fused"] = float(m.score_free_loss(**inp)), float(m.fused_loss(**inp))
    for _ in range(10):                                  # warm-up: plans, LDS attributes, the allocator
        free()
        fused()
        if dtype is not None:
            free16()
    for key, step in (("score_free_peak_mib", free), ("fused_peak_mib", fused)):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        gc.collect()                                     # what an earlier run left in reference cycles is not this step's
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res[key] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20      # above what was live before the step
    res["score_free_ms"], res["fused_ms"] = [], []
    if dtype is not None:
        res["score_free16_ms"] = []
    for _ in range(repeats):                             # alternate, so that drift hits all alike
        res["score_free_ms"].append(window_ms(free, window))
        res["fused_ms"].append(window_ms(fused, window))
        if dtype is not None:
            res["score_free16_ms"].append(window_ms(free16, window))
    for k in ("score_free", "fused") + (("score_free16",) if dtype is not None else ()):
        res[k + "_median_ms"] = statistics.median(res[k + "_ms"])
        res[k + "_spread_ms"] = max(res[k + "_ms"]) - min(res[k + "_ms"])
    res["step_time_ratio"] = res["score_free_median_ms"] / res["fused_median_ms"]      # below 1: score_free_loss is faster
    res["faster_beyond_spread"] = min(res["fused_ms"]) > max(res["score_free_ms"])
    res["slower_beyond_spread"] = min(res["score_free_ms"]) > max(res["fused_ms"])
    if dtype is not None:
        res["dtype"] = str(dtype)
        res["step16_time_ratio_to_score_free"] = res["score_free16_median_ms"] / res["score_free_median_ms"]
        res["step16_time_ratio_to_fused"] = res["score_free16_median_ms"] / res["fused_median_ms"]
    return res


def kernels(dtype=None, E=E):
    g = torch.Generator().manual_seed(3)
    R = B * L
    projected, table = torch.randn(R, E, generator=g).cuda(), (torch.randn(V, E, generator=g) * 0.1).cuda()
    bias, extra = torch.randn(V, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    targets = torch.randint(0, V, (R,), generator=g).cuda()
    g_norm, g_picked = torch.randn(R, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    stats = ops.projection_loss(projected, table, bias, extra, targets)[2]
    out = {"R": R, "V": V, "E": E}
    entries = [("projection_loss", 1, lambda: ops.projection_loss(projected, table, bias, extra, targets)),
               ("projection_loss_backward", 4,
                lambda: ops.projection_loss_backward(projected, table, bias, extra, targets, stats, g_norm, g_picked))]
    if dtype is not None:
        entries += [("projection_loss16", 1,
                     lambda: ops.projection_loss(projected, table, bias, extra, targets, inputs=dtype)),
                    ("projection_loss16_backward", 4,
                     lambda: ops.projection_loss_backward(projected, table, bias, extra, targets, stats, g_norm, g_picked,
                                                          inputs=dtype))]
    for name, passes, fn in entries:
        ms, flop = median_ms(fn), 2.0 * passes * R * V * E
        out[name] = {"ms": ms, "flop": flop, "tflops": flop / (ms * 1e-3) / 1e12,
                     "frac_of_fp32_matrix_peak": flop / (ms * 1e-3) / 1e12 / PEAK_FP32_MATRIX_TFLOPS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--dtype", choices=("bfloat16", "float16"), default=None)
    ap.add_argument("--dim", type=int, default=E)
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype) if args.dtype else None
    out = {"window_s": args.window, "repeats": args.repeats, "kernels": kernels(dtype, args.dim)}
    if not args.kernels_only:
        out["runs"] = [steps(p, args.window, args.repeats, dtype, args.dim) for p in (0.0, 0.2)]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
