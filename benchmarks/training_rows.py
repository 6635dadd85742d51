"""fp32 against 16-bit message and gradient rows in the GGNN edge-form training step (ptgnn_amd/precision.py
`half_messages(training=True)`; csrc/segment_reduce16.hip, the 16-bit-source / 16-bit-store forms of
csrc/edge_gemm16.hip, csrc/edge_wgrad16.hip) in one process, at a cfg3-like layer shape (E = 625 k edges, N = 116 k nodes,
T = 17 edge types, H = M = 128) and at the 256-wide last layer, bf16, p in {0, 0.1}: the aggregation, the spread, the two
gradient GEMMs and the producer alone -- three repeats of `--steps` launches per mode, interleaved, one HIP-event bracket
per repeat, medians, next to the HBM floors of their byte counts at 8 TB/s -- then one layer's forward + backward under
`matrix_inputs(bfloat16, edge_training=True)` with and without the keyword.  The baseline of every ratio is the same
process without the keyword, which is what the parent commit runs.  The record behind profiles/training_rows_notes.md:

    python -m benchmarks.training_rows [--out profiles/training_rows_bench.json] [--steps 5]
"""
import argparse
import json

import torch

import ptgnn_amd
from benchmarks.edge_inputs import DEV, HBM_BYTES_PER_S, interleaved
from ptgnn_amd import layers as L, ops

BF16 = torch.bfloat16
N, E, T = 115772, 625130, 17


def _floor_ms(nbytes):
    return round(nbytes / HBM_BYTES_PER_S * 1e3, 5)


def _graph(seed):
    g = torch.Generator().manual_seed(seed)
    counts = [E // T + (1 if t < E % T else 0) for t in range(T)]
    return [(torch.randint(0, N, (c,), generator=g).to(DEV), torch.randint(0, N, (c,), generator=g).to(DEV))
            for c in counts]


def launches(adj, plan, H, M, p, reduce, steps):
    g = torch.Generator().manual_seed(H + M)
    x = torch.randn(N, H, generator=g).to(DEV)
    ws = [(torch.randn(M, H, generator=g) * (2.0 / (H + M)) ** 0.5).to(DEV) for _ in range(T)]
    wts = [w.t().contiguous() for w in ws]
    w16, wt16 = torch.stack(ws).to(BF16).contiguous(), torch.stack(wts).to(BF16).contiguous()
    ident = [(i, i) for i in plan.identity_index()]
    bits = ops.dropout_bitmask(E, H, p, 7, DEV) if p else None
    fwd, bwd = ((1, p, 7), (2, p, 7)) if p else (None, None)
    kw = {"mask_bits": bits, "inputs": BF16}
    go = torch.randn(N, M, generator=g).to(DEV)
    with torch.no_grad():
        m32 = ops.edge_linear(x, adj, ws, False, dropout=fwd, rounded=w16, **kw)
        m16 = ops.edge_linear(x, adj, ws, False, dropout=fwd, rounded=w16, rows=BF16, **kw)
        arg = ops.gather_reduce(m32, plan, M, reduce, return_arg=True, type_bits=0, col=plan.perm)[1] \
            if reduce in ("max", "min") else None
        gm32 = ops.segment_spread(go, arg, plan)
        gm16 = ops.segment_spread16(go, arg, plan, reduce, BF16)
        fns = {
            "producer_rows32": lambda: ops.edge_linear(x, adj, ws, False, dropout=fwd, rounded=w16, **kw),
            "producer_rows16": lambda: ops.edge_linear(x, adj, ws, False, dropout=fwd, rounded=w16, rows=BF16, **kw),
            "aggregation_rows32": lambda: ops.gather_reduce(m32, plan, M, reduce, return_arg=arg is not None, type_bits=0,
                                                            col=plan.perm),
            "aggregation_rows16": lambda: ops.segment_reduce16(m16, plan, reduce, return_arg=arg is not None),
            "spread_rows32": lambda: ops.segment_spread(go, arg, plan),
            "spread_rows16": lambda: ops.segment_spread16(go, arg, plan, reduce, BF16),
            "input_grad_rows32": lambda: ops.edge_linear(gm32, ident, wts, False, dropout=bwd, rounded=wt16, **kw),
            "input_grad_rows16": lambda: ops.edge_linear(gm16, ident, wts, False, dropout=bwd, rounded=wt16, rows=BF16, **kw),
            "weight_grad_rows32": lambda: ops.edge_weight_grad(x, adj, gm32, False, p, 7, **kw),
            "weight_grad_rows16": lambda: ops.edge_weight_grad(x, adj, gm16, False, p, 7, **kw)}
        res = {"shape": f"H={H} M={M} T={T} E={E} N={N} p={p} {reduce}", "launches": interleaved(fns, steps)}
    a = 4 if arg is not None else 0
    res["hbm_floor_ms"] = {
        "producer_rows32": _floor_ms(E * (4 * H + 4 * M)), "producer_rows16": _floor_ms(E * (4 * H + 2 * M)),
        "aggregation_rows32": _floor_ms(E * (4 * M + 4) + N * M * (4 + a)),
        "aggregation_rows16": _floor_ms(E * (2 * M + 4) + N * M * (4 + a)),
        "spread_rows32": _floor_ms(E * (4 * M + 8) + N * M * (4 + a)),
        "spread_rows16": _floor_ms(E * (2 * M + 8) + N * M * (4 + a)),
        "input_grad_rows32": _floor_ms(E * (4 * M + 4 * H)), "input_grad_rows16": _floor_ms(E * (2 * M + 2 * H)),
        "weight_grad_rows32": _floor_ms(E * (4 * M + 4 * H)), "weight_grad_rows16": _floor_ms(E * (2 * M + 4 * H))}
    med = {k: v["median_ms"] for k, v in res["launches"].items()}
    res["rows16_over_rows32"] = {k[:-7]: round(med[k] / med[k[:-2] + "32"], 4) for k in med if k.endswith("rows16")}
    res["fraction_of_hbm_peak"] = {k: round(res["hbm_floor_ms"][k] / v, 3) for k, v in med.items()}
    return res


def layer_step(adj, H, p, reduce, steps):
    torch.manual_seed(3)
    layer = L.GatedMessagePassingLayer(H, H, T, reduce, dropout_rate=p).to(DEV).train()
    x = torch.randn(N, H, device=DEV)
    go = torch.randn(N, H, device=DEV)
    feats = [torch.empty(int(s.shape[0]), 0, device=DEV) for s, _ in adj]

    def step(on):
        def run():
            with ptgnn_amd.matrix_inputs(BF16, edge_training=True), ptgnn_amd.half_messages(on, training=on):
                xs = x.detach().requires_grad_(True)
                layer.zero_grad()
                layer(xs, adj, None, {}, {}, feats).backward(go)
        return run
    res = interleaved({"layer_rows32": step(False), "layer_rows16": step(True)}, steps)
    return {"launches": res, "rows16_over_rows32": round(res["layer_rows16"]["median_ms"] / res["layer_rows32"]["median_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    adj = _graph(11)
    plan = ops.plan_for(adj, N)
    record = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "steps": args.steps, "cases": []}
    for H in (128, 256):
        for p in (0.0, 0.1):
            case = launches(adj, plan, H, H, p, "max", args.steps)
            case["layer_forward_backward"] = layer_step(adj, H, p, "max", args.steps)
            record["cases"].append(case)
            print(json.dumps({"shape": case["shape"], "rows16_over_rows32": case["rows16_over_rows32"],
                              "layer": case["layer_forward_backward"]["rows16_over_rows32"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
