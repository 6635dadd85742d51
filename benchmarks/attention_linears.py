"""The attention layer's three training Linears (summarisation 256 -> 256, intermediate 256 -> 1024 + ReLU, output
1024 -> 256, the first and last with dropout and a residual) on the panel-form 16-bit Linear
(`ptgnn_amd.set_attention_training(True, linears=True)`; csrc/panel_linear16.hip, the masked form of csrc/wgrad16.hip)
against the fp32 node's launches and the existing 16-bit Linear in one process, at the batch of
profiles/attention_training_notes.md (48 graphs / ~107 k nodes, D 256, intermediate 1024) and with the timing method of
benchmarks/attention_inputs.py: HIP events, median of 21 after warm-up.

Per dropout rate (0 and 0.1), 16-bit type and Linear: the forward, input-gradient and weight-gradient launch of the new
route; what the fp32 node runs for the same work (Linear + torch's dropout + torch's residual add; act_dropout_backward;
Linear; weight gradient); `ops.linear(..., inputs=dt)` (k_half_linear) for the forward.  Then the layer's training step
under `attention_training(linears=True)`, under `attention_training()` and in fp32.  The panel width the launches use is
the library's (PTGNN_AMD_PANEL16_KT=32|64 in the environment selects the other one for the KT comparison of the notes).
The record behind profiles/attention_linears_notes.md:

    python -m benchmarks.attention_linears [--out profiles/attention_linears_bench.json] [--reps 21]
"""
import argparse
import json
import os

import torch

import ptgnn_amd
from benchmarks.attention_inputs import D, DEV, DK, DV, HEADS, INTER, MAXN, MODES, t_med
from ptgnn_amd import layers as L, ops

RATES = (0.0, 0.1)
SEED = 1234
# (name, k, n_out, act, bias, dropout follows, residual follows)
LINEARS = (("summarisation", D, D, None, False, True, True), ("intermediate", D, INTER, "relu", True, False, False),
           ("output", INTER, D, None, True, True, True))


def run_linear(spec, n, p_layer, dt, reps, g):
    name, k, n_out, act, has_bias, drops, adds = spec
    p = p_layer if drops else 0.0
    x, grad = torch.randn(n, k, generator=g).to(DEV), torch.randn(n, n_out, generator=g).to(DEV)
    add = torch.randn(n, n_out, generator=g).to(DEV) if adds else None
    w = ((torch.rand(n_out, k, generator=g) * 2 - 1) * (6.0 / (n_out + k)) ** 0.5).to(DEV)
    b = (torch.randn(n_out, generator=g) * 0.1).to(DEV) if has_bias else None
    wt, w16, wt16 = w.t().contiguous(), w.to(dt), w.t().contiguous().to(dt)
    want_act = act is not None and p > 0
    y = ops.linear(x, w, b, act=act)
    keep = torch.rand(n, n_out, device=DEV) >= p if p > 0 else None
    scale = 1.0 / (1.0 - p)

    def fp32_forward():
        out = ops.linear(x, w, b, act=act)
        out = torch.ops.aten.native_dropout(out, p, True)[0] if p > 0 else out
        return out + add if adds else out

    def fp32_grad_input():
        g1 = ops.act_dropout_backward(grad, y, keep, scale, act) if (p > 0 or act) else grad
        return ops.linear(g1, wt)

    g1 = ops.act_dropout_backward(grad, y, keep, scale, act)
    res = {
        "k": k, "n_out": n_out, "p": p, "gflop_per_gemm": 2e-9 * n * k * n_out,
        "forward_ms": t_med(lambda: ops.panel_linear16(x, w, b, act, dt, p=p, seed=SEED, addend=add, want_act=want_act,
                                                       rounded=w16), reps),
        "grad_input_ms": t_med(lambda: ops.panel_linear16_grad_input(grad, y, wt, act, dt, p=p, seed=SEED, rounded=wt16),
                               reps),
        "weight_grad_ms": t_med(lambda: ops.half_linear_weight_grad_masked(x, grad, y, act, dt, p=p, seed=SEED,
                                                                            want_bias=has_bias), reps),
        "fp32_forward_ms": t_med(fp32_forward, reps),
        "fp32_grad_input_ms": t_med(fp32_grad_input, reps),        # act_dropout_backward's pass is counted here, once
        "fp32_weight_grad_ms": t_med(lambda: ops.linear_weight_grad(x, g1, want_bias=has_bias), reps),
        "half_linear_forward_ms": t_med(lambda: ops.linear(x, w, b, act=act, inputs=dt, rounded=w16), reps),
    }
    for key in ("forward", "grad_input", "weight_grad"):
        res[key + "_over_float32"] = res[key + "_ms"] / res["fp32_" + key + "_ms"]
    res["forward_over_half_linear"] = res["forward_ms"] / res["half_linear_forward_ms"]
    return name, res


def main(out=None, reps=21):
    g = torch.Generator().manual_seed(3)
    sizes = (torch.rand(48, generator=g) * 1600 + 1620).long().tolist()       # ~107 k nodes in 48 graphs
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    n = idx.shape[0]
    x = torch.randn(n, D, generator=g).to(DEV)
    res = {"device": torch.cuda.get_device_name(0), "N": n, "G": len(sizes), "D": D, "intermediate": INTER,
           "panel_kt": os.environ.get("PTGNN_AMD_PANEL16_KT", "library default"),
           "timing": f"HIP events, median of {reps} after 3 warm-up calls", "rates": {}}
    for p in RATES:
        torch.manual_seed(1)
        module = L.MultiHeadSelfAttentionMessagePassing(D, DK, DV, D, INTER, HEADS, dropout_rate=p,
                                                        max_num_nodes=MAXN).to(DEV).train()

        def step():
            module.zero_grad(set_to_none=True)
            module(x, [], idx, {}, {}, []).square().sum().backward()

        entry = {"float32": {"layer_step_ms": t_med(step, reps)}}
        for mode, dt in MODES[1:]:
            entry[mode] = dict(run_linear(spec, n, p, dt, reps, g) for spec in LINEARS)
            with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training():
                entry[mode]["layer_step_plain_switch_ms"] = t_med(step, reps)
            with ptgnn_amd.matrix_inputs(dt), ptgnn_amd.attention_training(linears=True):
                before = ops.launch_counts(panel16=True)
                step()
                since = ops.launches_since(before)
                assert since.get("panel_linear16") == 3 and since.get("panel_linear16_grad_input") == 3, since
                entry[mode]["layer_step_ms"] = t_med(step, reps)
            entry[mode]["layer_step_over_plain_switch"] = entry[mode]["layer_step_ms"] / entry[mode]["layer_step_plain_switch_ms"]
            entry[mode]["layer_step_over_float32"] = entry[mode]["layer_step_ms"] / entry["float32"]["layer_step_ms"]
        res["rates"][str(p)] = entry
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/attention_linears_bench.json")
    parser.add_argument("--reps", type=int, default=21)
    args = parser.parse_args()
    main(args.out, args.reps)
