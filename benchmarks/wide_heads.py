"""The attention pool and the copy scores past 8 heads on the matrix-core kernels (`ptgnn_amd.set_wide_heads(True)`;
csrc/wide_heads.hip) against the composed operator sequence the same shapes take with the switch off, in one process,
timed with HIP events around whole calls (median, minimum and maximum after 3 warm-up calls); the two routes of a
comparison are timed alternately, one call each per repetition.

Decoder shapes: B = 50 samples, Dm = H = 256, L in {16, 32, 64} decoding steps, ~200 and ~2 000 memories per sample.
Per shape: the four calls alone (pool, pool backward, scores, scores backward -- each the chunk-table launch, the chunk
kernel and the merge / fold launch with the wrapper's workspace handling, so a call's time, not a kernel's) with their
FLOPs against the 157 TF fp32-MFMA peak and their bytes against 8 TB/s; the decoder's attention (pool + copy scores,
forward and backward) with the switch on and off; the decoder's training step (`fused_loss`, dropout 0 and 0.2) on and off.  Then the multi-head reducer
at D = 256, 16 heads, ~116 k elements over 50 samples, training step on and off.  The record behind
profiles/wide_heads_notes.md:

    python -m benchmarks.wide_heads [--out profiles/wide_heads_bench.json] [--reps 11]
"""
import argparse
import json

import torch

import ptgnn_amd
from benchmarks.attention_inputs import DEV
from ptgnn_amd import ops, reduceops as R, sequence

B, DM, H, V, E = 50, 256, 256, 5000, 128
PEAK_FLOPS, PEAK_BYTES = 157e12, 8e12


def timed(fns, reps):
    """[(median, min, max) ms] of each of `fns`, called in turn within every repetition (3 warm-up rounds first)."""
    for _ in range(3):
        for fn in fns:
            fn()
    evs = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            evs[k].append((s, e))
    torch.cuda.synchronize()
    out = []
    for pairs in evs:
        ms = sorted(a.elapsed_time(b) for a, b in pairs)
        out.append((ms[reps // 2], ms[0], ms[-1]))
    return out


def roofline(stats, flops, nbytes):
    """A call's share of the least time the hardware could take for its kernel's work (call-level: see the module text)."""
    ms = stats[0]
    least = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e3
    return {"ms": ms, "min_ms": stats[1], "max_ms": stats[2], "gflop": flops * 1e-9, "mbytes": nbytes * 1e-6,
            "tflops": flops / ms * 1e-9,
            "gbytes_per_s": nbytes / ms * 1e-6, "bound": "flops" if flops / PEAK_FLOPS > nbytes / PEAK_BYTES else "bytes",
            "share_of_bound": least / ms}


def kernels(x, plan, L, reps, g):
    n, d = x.shape
    u = (torch.randn(B, L, d, generator=g) / d ** 0.5).to(DEV)
    gp, gs, gl = (torch.randn(*s, generator=g).to(DEV) for s in ((B, L, d), (n, L), (B, L)))
    pooled, stats = ops.wide_heads_pool(x, u, plan)
    scores, lse = ops.wide_heads_scores(x, u, plan)
    rows, vecs = 4.0 * n * d, 4.0 * B * L * d
    t = timed([lambda: ops.wide_heads_pool(x, u, plan),
               lambda: ops.wide_heads_pool_backward(x, u, plan, pooled, stats, gp),
               lambda: ops.wide_heads_scores(x, u, plan),
               lambda: ops.wide_heads_scores_backward(x, u, plan, scores, lse, gs, gl)], 3 * reps)
    return {"pool": roofline(t[0], 4.0 * n * L * d, rows + 2 * vecs),
            "pool_backward": roofline(t[1], 12.0 * n * L * d, 2 * rows + 4 * vecs),
            "scores": roofline(t[2], 2.0 * n * L * d, rows + vecs + 4.0 * n * L),
            "scores_backward": roofline(t[3], 4.0 * n * L * d, 2 * rows + 2 * vecs + 8.0 * n * L)}


def on_off(fn, reps, families):
    def route(on):
        def call():
            with ptgnn_amd.wide_heads(on):
                fn()
        return call

    for on in (False, True):
        before = ops.launch_counts(wide_heads=True)
        route(on)()
        assert all((f in ops.launches_since(before)) == on for f in families), (on, ops.launches_since(before))
    off, on = timed([route(False), route(True)], reps)
    return {"off_ms": off[0], "off_min_ms": off[1], "off_max_ms": off[2], "on_ms": on[0], "on_min_ms": on[1],
            "on_max_ms": on[2], "on_over_off": on[0] / off[0]}


def decoder_shape(per_sample, L, reps, g):
    sizes = (torch.rand(B, generator=g) * per_sample + per_sample // 2).long().tolist()
    index = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    index = index[torch.randperm(index.shape[0], generator=g)].to(DEV)
    n = index.shape[0]
    x = torch.randn(n, DM, generator=g).to(DEV)
    plan = ops.plan_for([(index, index)], B)
    res = {"memories": n, "L": L, "kernels": kernels(x, plan, L, reps, g)}
    tokens = torch.randint(2, V, (B, L + 1), generator=g).to(DEV)
    inputs = dict(input_memories=x, input_memories_origin_idx=index,
                  initial_states=torch.randn(B, H, generator=g).to(DEV), target_token_ids=tokens,
                  copyable_elements_idxs=torch.arange(0, n * L, max(1, n * L // 400), dtype=torch.int64, device=DEV)[:B * L],
                  copyable_elements_sample_idxs=None, target_lengths=torch.full((B,), L, dtype=torch.int64, device=DEV))
    inputs["copyable_elements_sample_idxs"] = index[inputs["copyable_elements_idxs"] // L] * L + \
        inputs["copyable_elements_idxs"] % L
    families = ("wide_heads_pool", "wide_heads_pool_backward", "wide_heads_scores", "wide_heads_scores_backward")
    for rate in (0.0, 0.2):
        torch.manual_seed(1)
        module = sequence.GruCopyingDecoder(V, E, H, DM, 0, rate).to(DEV).train()
        states = torch.randn(B, L, H, generator=g).to(DEV).requires_grad_(True)
        xg = x.clone().requires_grad_(True)

        def attend():
            module.zero_grad(set_to_none=True)
            a, c, t = module._GruCopyingDecoder__attend(states, xg, index, plan)
            (a.sum() + c.sum() + t.sum()).backward()

        def step():
            module.zero_grad(set_to_none=True)
            module.fused_loss(**inputs).backward()

        res[f"dropout_{rate}"] = {"attention_forward_backward": on_off(attend, reps, families),
                                  "fused_loss_step": on_off(step, reps, families)}
    return res


def reducer(reps, g):
    D, heads = 256, 16
    sizes = (torch.rand(B, generator=g) * 1600 + 1520).long().tolist()          # ~116 k elements in 50 samples
    idx = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(DEV)
    x = torch.randn(idx.shape[0], D, generator=g).to(DEV).requires_grad_(True)
    torch.manual_seed(2)
    module = R.MultiheadSelfAttentionVarSizedElementReduce(D, D, 128, heads, R.SimpleVarSizedElementReduce("max")).to(DEV)

    def step():
        module.zero_grad(set_to_none=True)
        x.grad = None
        module(R.ElementsToSummaryRepresentationInput(x, idx, B)).square().sum().backward()

    return dict(elements=idx.shape[0], D=D, heads=heads,
                training_step=on_off(step, reps, ("wide_heads_pool", "wide_heads_pool_backward")))


def main(out=None, reps=11, lengths=(16, 32, 64), memories=(200, 2000)):
    g = torch.Generator().manual_seed(7)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "Dm": DM, "H": H, "V": V, "E": E,
           "timing": f"HIP events around whole calls, median / min / max of {reps} (single calls: {3 * reps}) after 3 warm-up "
                     "rounds; compared routes alternate within a repetition", "decoder": [], "reducer": reducer(reps, g)}
    for per_sample in memories:
        for L in lengths:
            res["decoder"].append(decoder_shape(per_sample, L, reps, g))
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default="profiles/wide_heads_bench.json")
    parser.add_argument("--reps", type=int, default=11)
    args = parser.parse_args()
    main(args.out, args.reps)
