"""Segment softmax / log-softmax / logsumexp timings: the fused node (`scatter.fused_softmax()`,
csrc/segment_softmax.hip) against the composed chain of segment reduces, gathers and torch operators the facade runs
with the switch off, in ONE process on the same inputs.  Not part of bench.py.

    python scripts/segment_softmax_bench.py [--out FILE] [--reps N] [--inner K] [--limit SECONDS] [--shapes a,b]

Per shape and kind, HIP events around `--inner` back-to-back calls, `--reps` such windows per route after warm-up, the two
routes alternating window by window; reported per call: median and the min .. max spread of the windows.
  * facade forward and forward + backward, switch on and off (both build the plan of the index, as an untouched ptgnn
    model's call does);
  * the fused ops alone over a held plan (`ops.segment_softmax`, + `ops.segment_softmax_backward`), and the forward's HBM
    floor 3 E D 4 bytes at 8 TB/s.
These windows are enqueue-bound at the small shapes (a fused forward is two launches behind ~35 us of Python); kernel
times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/segment_softmax_bench.py --shapes X`.
Every shape runs under its own time limit (--limit): a shape that overruns ends the run, nothing is started after it."""
import argparse
import json
import os
import signal
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import ops, scatter as S  # noqa: E402

PEAK_TBPS = 8.0
KINDS = ("softmax", "log_softmax", "logsumexp")
# name: (elements, columns, segments)
SHAPES = {"varmisuse": (100_000, 1, 10_000), "decoder": (10_000, 8, 50), "summariser": (116_000, 8, 50),
          "wide": (10_000, 512, 50)}


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    return s, e


def alternate(fns, reps, inner):
    """{name: (median, min, max) ms per call} of the callables, warmed up, their windows interleaved."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    evs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            evs[k].append(window(fn, inner))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in evs.items():
        t = sorted(a.elapsed_time(b) / inner for a, b in pairs)
        out[k] = (t[len(t) // 2], t[0], t[-1])
    return out


def shape_run(name, reps, inner):
    E, D, n = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    index = torch.randint(0, n, (E,), generator=g).cuda()
    x = (torch.randn(E, D, generator=g) * 3).cuda()
    xg = x.clone().requires_grad_(True)
    plan = ops.build_plan([(index, index)], n)
    res = {"shape": name, "E": E, "D": D, "segments": n, "floor_us": 3.0 * E * D * 4 / (PEAK_TBPS * 1e12) * 1e6}
    for kind in KINDS:
        call = getattr(S, "scatter_" + kind)

        def facade(on, src, backward):
            with S.fused_softmax(on):
                out = call(src, index, dim=0, dim_size=n)
            if backward:
                src.grad = None
                out.clamp(min=-50).sum().backward()
            return out

        with torch.no_grad():
            diff = (facade(True, x, False) - facade(False, x, False)).nan_to_num(0.0, 0.0, 0.0).abs().max()
        out, _ = ops.segment_softmax(x, index, plan, kind)
        grad = torch.randn_like(out)
        saved = dict(x=x, lse=out) if kind == "logsumexp" else dict(y=out)
        t = alternate({"fused_fwd": lambda: facade(True, x, False), "composed_fwd": lambda: facade(False, x, False),
                       "fused_fwd_bwd": lambda: facade(True, xg, True), "composed_fwd_bwd": lambda: facade(False, xg, True),
                       "op_fwd": lambda: ops.segment_softmax(x, index, plan, kind),
                       "op_bwd": lambda: ops.segment_softmax_backward(grad, index, plan, kind, **saved)}, reps, inner)
        res[kind] = {k: {"median_us": v[0] * 1e3, "min_us": v[1] * 1e3, "max_us": v[2] * 1e3} for k, v in t.items()}
        res[kind]["max_abs_fused_vs_composed"] = float(diff)
        res[kind]["op_fwd_over_floor"] = t["op_fwd"][0] * 1e3 / res["floor_us"]
    return res


def overran(signum, frame):
    raise TimeoutError("a shape overran its time limit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--limit", type=int, default=90)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_softmax_bench: needs a GPU (timings on a CPU say nothing)")
    signal.signal(signal.SIGALRM, overran)
    runs = []
    for name in args.shapes.split(","):
        signal.alarm(args.limit)
        runs.append(shape_run(name, args.reps, args.inner))     # a TimeoutError ends the process: nothing runs after it
        signal.alarm(0)
    line = json.dumps({"reps": args.reps, "inner": args.inner, "runs": runs})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
