"""The decoder's fused loss against its `forward` (GruCopyingDecoder at the shapes of scripts/decoder_bench.py: B = 64,
L = 7, H = Dm = 128, E = 256, V = 20 000, 100 .. 500 memories per sample; dropout 0 and 0.2).  Not part of bench.py.

    python scripts/graph2seq_bench.py [--out FILE] [--window SECONDS] [--repeats N]

A training step (loss + backward w.r.t. the memories, the initial states and every weight) of `fused_loss` and of
`forward` on the SAME module in the same process: after a warm-up the two alternate, each timed with device events over a
window of at least --window seconds of its own steps, --repeats times, so the spread is visible next to the difference.
Then the three kernels of csrc/vocab_loss.hip alone (device events around the wrapper calls, median) with their achieved
bytes/s over the formula bytes of DESIGN.md:
    vocab_loss            R V 4 + V 4                                read once
    vocab_loss_backward   2 R V 4 + V 4 + 2 ceil(R / 8) V 4          read + written + grad_bias partials
    copy_loss_finish      28 B L + 12 B
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/graph2seq_bench.py`."""
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
from ptgnn_amd import ops, sequence  # noqa: E402

PEAK_TBPS = 8.0


def window_ms(step, seconds):
    """Mean milliseconds of `step` over a window of at least `seconds` of device time."""
    total, count, chunk = 0.0, 0, 10
    while total < seconds * 1e3:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(chunk):
            step()
        e.record()
        e.synchronize()
        total += s.elapsed_time(e)
        count += chunk
    return total / count


def median_ms(fn, reps=31):
    for _ in range(5):
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


def steps(dropout, window, repeats):
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

    fused, plain = step_of(m.fused_loss), step_of(m.forward)
    res = {"dropout": dropout, "I": int(inp["input_memories"].shape[0]), "B": B, "L": L, "V": V, "E": E, "H": H}
    if dropout == 0.0:
        with torch.no_grad():
            res["loss_fused"], res["loss_forward"] = float(m.fused_loss(**inp)), float(m(**inp))
    for _ in range(10):                                  # warm-up: plans, LDS attributes, the allocator
        fused()
        plain()
    for key, step in (("fused_peak_mib", fused), ("forward_peak_mib", plain)):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        gc.collect()                                     # what an earlier run left in reference cycles is not this step's
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res[key] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20      # above what was live before the step
    res["fused_ms"], res["forward_ms"] = [], []
    for _ in range(repeats):                             # alternate, so that drift hits both alike
        res["fused_ms"].append(window_ms(fused, window))
        res["forward_ms"].append(window_ms(plain, window))
    for k in ("fused", "forward"):
        res[k + "_median_ms"] = statistics.median(res[k + "_ms"])
        res[k + "_spread_ms"] = max(res[k + "_ms"]) - min(res[k + "_ms"])
    res["speedup"] = res["forward_median_ms"] / res["fused_median_ms"]
    res["faster_beyond_spread"] = min(res["forward_ms"]) > max(res["fused_ms"])
    return res


def kernels():
    g = torch.Generator().manual_seed(3)
    R = B * L
    scores = torch.randn(R, V, generator=g).cuda()
    bias, extra = torch.randn(V, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    targets = torch.randint(0, V, (R,), generator=g).cuda()
    g_norm, g_picked = torch.randn(R, generator=g).cuda(), torch.randn(R, generator=g).cuda()
    norm, picked, stats = ops.vocab_loss(scores, bias, extra, targets)
    out = {"R": R, "V": V}
    for name, nbytes, fn in (
            ("vocab_loss", 4.0 * R * V + 4.0 * V, lambda: ops.vocab_loss(scores, bias, extra, targets)),
            ("vocab_loss_backward", 8.0 * R * V + 4.0 * V + 8.0 * ((R + 7) // 8) * V,
             lambda: ops.vocab_loss_backward(scores, bias, extra, targets, stats, g_norm, g_picked))):
        ms = median_ms(fn)
        out[name] = {"ms": ms, "bytes": nbytes, "tbps": nbytes / (ms * 1e-3) / 1e12,
                     "frac_of_peak": nbytes / (ms * 1e-3) / 1e12 / PEAK_TBPS}
    gen, copied = picked.reshape(B, L), torch.randn(B, L, generator=g).cuda()
    lengths = torch.randint(1, L + 1, (B,), generator=g).cuda()
    rowptr = torch.arange(R + 1, dtype=torch.int32).cuda()
    ms = median_ms(lambda: ops.copy_loss_finish(gen, copied, rowptr, targets.reshape(B, L), UNK, lengths))
    nbytes = 28.0 * R + 12.0 * B
    out["copy_loss_finish"] = {"ms": ms, "bytes": nbytes, "tbps": nbytes / (ms * 1e-3) / 1e12}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    out = {"window_s": args.window, "repeats": args.repeats, "kernels": kernels(),
           "runs": [steps(0.0, args.window, args.repeats), steps(0.2, args.window, args.repeats)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
