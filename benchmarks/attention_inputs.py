"""The attention layer's block attention and inference forward with fp32 against 16-bit matrix inputs
(ptgnn_amd/precision.py, `attention=True`; csrc/block_attention16.hip) in one process, on the two batches and with the
timing method of profiles/selfatt_notes.md: 48 graphs / 107 278 nodes and 4 000 graphs / 113 825 nodes, D = 256, 8 heads,
dk = dv = 32, intermediate 1024, max_num_nodes 250; HIP events, median of 21 after warm-up.  The baseline is the fp32
kernel of the same run.

Per batch and mode: the attention op alone (with its share of the matrix-core peak of the mode: 157.3 TF for the fp32
MFMA, 16 x that for the 16-bit ones) and the layer's inference forward.  Also, reported and not asserted, at full size:
the largest |got - rounded| / bound of tests/attention_inputs_cases.py (restated here: benchmarks import nothing from
tests/) and the largest |got - exact|, against float64 restatements on the device.  The record behind
profiles/attention_inputs_notes.md:

    python -m benchmarks.attention_inputs [--out profiles/attention_inputs_bench.json] [--reps 21]
"""
import argparse
import json
import math

import torch

import ptgnn_amd
from ptgnn_amd import layers as L, ops

DEV = torch.device("cuda")
MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))
PEAK_TF = {"float32": 157.3, "bfloat16": 16 * 157.3, "float16": 16 * 157.3}
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
TOL = 1e-5
D, HEADS, DK, DV, INTER, MAXN = 256, 8, 32, 32, 1024, 250


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


def attention64(kqv, bounds, dt=None):
    """float64 attention on the device: dt None = exact operands, else k, q, v rounded to dt and P unrounded.
    -> out [N, heads dv], weight = (P |rnd(V)|) [N, heads dv], window length per row [N]."""
    n = kqv.shape[0]
    x = (kqv if dt is None else kqv.to(dt)).double().reshape(n, HEADS, 2 * DK + DV)
    out, weight = torch.empty(n, HEADS, DV, dtype=torch.float64, device=DEV), \
        torch.empty(n, HEADS, DV, dtype=torch.float64, device=DEV)
    length = torch.empty(n, dtype=torch.float64, device=DEV)
    for lo, hi in bounds:
        k, q, v = x[lo:hi, :, :DK], x[lo:hi, :, DK:2 * DK], x[lo:hi, :, 2 * DK:]
        p = torch.softmax(torch.einsum("khd,vhd->khv", k, q) / math.sqrt(DK), dim=-1)
        out[lo:hi] = torch.einsum("khv,vhd->khd", p, v)
        weight[lo:hi] = torch.einsum("khv,vhd->khd", p, v.abs())
        length[lo:hi] = hi - lo
    return out.reshape(n, -1), weight.reshape(n, -1), length, float(x[..., 2 * DK:].abs().max())


def numerics(kqv, bounds, windows):
    exact = attention64(kqv, bounds)[0]
    res = {"float32_max_abs_vs_exact": float((ops.block_attention(kqv, windows, MAXN, HEADS, DK, DV)[0].double()
                                              - exact).abs().max())}
    for name, dt in MODES[1:]:
        rounded, weight, length, vmax = attention64(kqv, bounds, dt)
        bound = UNIT[dt] * weight + (length * TINY[dt] * vmax).unsqueeze(1) + TOL * max(1.0, float(rounded.abs().max()))
        got = ops.block_attention(kqv, windows, MAXN, HEADS, DK, DV, inputs=dt)[0].double()
        res[name] = {"max_err_over_bound_vs_rounded": float(((got - rounded).abs() / bound).max()),
                     "max_abs_vs_exact": float((got - exact).abs().max()),
                     "max_abs_exact_vs_rounded": float((exact - rounded).abs().max())}
    return res


def run_batch(name, sizes, module, reps):
    g = torch.Generator().manual_seed(7)
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    n = idx.shape[0]
    x = torch.randn(n, D, generator=g).to(DEV)
    bounds = window_bounds(sizes)
    flop = float(sum(HEADS * 2 * (hi - lo) ** 2 * (DK + DV) for lo, hi in bounds))
    res = {"batch": name, "N": n, "G": len(sizes), "windows": len(bounds), "attention_flop": flop, "attention": {},
           "layer_inference": {}}
    with torch.no_grad():
        windows = ops.attention_windows(L._index_plan(idx, len(sizes)), MAXN)
        kqv = torch.randn(n, HEADS * (2 * DK + DV), generator=g).to(DEV)
        for mode, dt in MODES:
            before = ops.launch_counts(aggregation=True, attention16=True)
            ops.block_attention(kqv, windows, MAXN, HEADS, DK, DV, inputs=dt)
            family = "block_attention" if dt == torch.float32 else "block_attention16"
            assert ops.launches_since(before) == {family: 1}
            ms = t_med(lambda: ops.block_attention(kqv, windows, MAXN, HEADS, DK, DV, inputs=dt), reps)
            tf = flop / (ms * 1e-3) / 1e12
            res["attention"][mode] = {"ms": ms, "tflops": tf, "frac_of_fp32_mfma_peak": tf / PEAK_TF["float32"],
                                      "frac_of_own_mfma_peak": tf / PEAK_TF[mode]}
            with ptgnn_amd.matrix_inputs(dt, attention=True):
                res["layer_inference"][mode] = {"ms": t_med(lambda: module(x, [], idx, {}, {}, []), reps)}
        for mode, _ in MODES[1:]:
            for key in ("attention", "layer_inference"):
                res[key][mode]["over_float32"] = res[key][mode]["ms"] / res[key]["float32"]["ms"]
        res["numerics_attention"] = numerics(kqv, bounds, windows)
    return res


def main(out=None, reps=21):
    torch.manual_seed(1)
    module = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, max_num_nodes=MAXN).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    big = (torch.rand(48, generator=g) * 1600 + 1620).long().tolist()       # ~107 k nodes in 48 graphs
    small = (torch.rand(4000, generator=g) * 30 + 14).long().tolist()       # ~114 k nodes in 4 000 graphs
    res = {"device": torch.cuda.get_device_name(0), "D": D, "heads": HEADS, "dk": DK, "dv": DV, "intermediate": INTER,
           "max_num_nodes": MAXN, "timing": f"HIP events, median of {reps} after 3 warm-up calls",
           "batches": [run_batch("graph2class_48", big, module, reps), run_batch("small_4000", small, module, reps)]}
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/attention_inputs_bench.json")
    parser.add_argument("--reps", type=int, default=21)
    args = parser.parse_args()
    main(args.out, args.reps)
