"""One beam-search call of GruCopyingDecoder at the shapes of benchmarks/greedy_decode.py (B = 50 samples, V = 20 000,
max_seq_len = 8, H = 128, E = 256, about 200 memories per sample; the same seeded module and inputs), for the beam widths
W = 1, 4, 8 -- on two routes, alternated in one process:

  device    `GruCopyingDecoder.beam_decode`: the loop on device tensors, one csrc/beam_step.hip call per step;
  host      a host beam loop restated here around `_compute_logprobs` (the only route before `beam_decode` existed, the
            analogue of benchmarks/greedy_decode.py's `host_loop`): the W slots of a sample as W rows of one call with the
            memories repeated per slot, torch.topk(100), three .cpu() copies, the Python dict merge per (memory, slot),
            the W best of a sample's pool and the next token / state tensors built on the host;

and `greedy_decode` on the same inputs in the same process as the yardstick.  The routes' results are compared before
timing and the comparison is part of the record (the weights are random, so a decision can sit closer than fp32
resolves).  5 warm-up calls per route, then 7 rounds of (10 device calls, 10 greedy calls, 2 host calls), every call
closed by a device synchronise; median / min / max of the rounds' per-call wall time, and the C-ABI launches of one step
of the device route.  The record behind profiles/beam_decode_notes.md:

    python -m benchmarks.beam_decode [--out profiles/beam_decode_bench.json]
"""
import argparse
import json
import math
import statistics

import numpy as np
import torch

from benchmarks.greedy_decode import B, DEV, END_ID, START_ID, T, TOP_K, UNK_ID, V, make_case, per_call_us, summary
from ptgnn_amd import ops

WIDTHS = (1, 4, 8)


def host_beam_loop(module, inputs, W):
    """Beam search over the dict of grucopydecoder.py:406-442 on extended ids, ordered as `beam_decode` documents."""
    x, index, h0 = inputs["input_memories"], inputs["input_memories_origin_idx"], inputs["initial_states"]
    I = x.shape[0]
    values = inputs["input_element_ids"].cpu().tolist()
    sample_of = index.cpu().tolist()
    x_rows = x.repeat(W, 1)                                         # the memories once per slot, slot-major
    rows = index.repeat(W) * W + torch.arange(W, device=DEV).repeat_interleave(I)
    h = h0.unsqueeze(1).expand(B, W, h0.shape[1]).reshape(B * W, -1).contiguous()
    feed = torch.full((B * W, 1), START_ID, device=DEV)
    scores = [[0.0] + [-math.inf] * (W - 1) for _ in range(B)]
    done = [[False] * W for _ in range(B)]
    history = [[[] for _ in range(W)] for _ in range(B)]
    with torch.no_grad():
        for _ in range(T):
            copy_logprobs, target_logprobs, state = module._compute_logprobs(h, x_rows, rows, feed)
            top_logprobs, top_ids = torch.topk(target_logprobs.squeeze(1), min(TOP_K, V), dim=-1)
            top_logprobs, top_ids = top_logprobs.cpu().numpy(), top_ids.cpu().numpy()
            copy_logprobs = copy_logprobs.squeeze(1).cpu().numpy().reshape(W, I)
            entries = [dict(zip(top_ids[r].tolist(), top_logprobs[r])) for r in range(B * W)]
            best = [set(top_ids[r, :W].tolist()) for r in range(B * W)]
            for j in range(W):
                for b, value, c in zip(sample_of, values, copy_logprobs[j]):
                    e = entries[b * W + j]
                    e[value] = np.logaddexp(e.get(value, -math.inf), c)
            parents, step = [], []
            for b in range(B):
                pool = []
                for j in range(W):
                    if done[b][j]:
                        pool.append((scores[b][j], j, 0, -1))
                    else:
                        pool += [(scores[b][j] + float(v), j, 0 if g in best[b * W + j] else 1, g)
                                 for g, v in entries[b * W + j].items()]
                chosen = sorted(pool, key=lambda c: (-c[0], c[1], c[2], c[3]))[:W]
                ends = [done[b][c[1]] or c[3] == END_ID for c in chosen]
                history[b] = [history[b][c[1]] + ([] if e else [c[3]]) for c, e in zip(chosen, ends)]
                scores[b], done[b] = [c[0] for c in chosen], ends
                parents += [b * W + c[1] for c in chosen]
                step += [END_ID if e else (c[3] if c[3] < V else UNK_ID) for c, e in zip(chosen, ends)]
            h = state.squeeze(0)[torch.tensor(parents, device=DEV)]
            feed = torch.tensor(step, device=DEV).unsqueeze(1)
    return history, scores


def main(out=None, rounds=7):
    module, inputs = make_case()

    def greedy():
        return module.greedy_decode(**inputs, start_id=START_ID, end_id=END_ID, max_seq_len=T, top_k=TOP_K)

    res = {"shape": dict(B=B, V=V, max_seq_len=T, memories=int(inputs["input_memories"].shape[0]), top_k=TOP_K), "widths": {}}
    for W in WIDTHS:
        def device():
            return module.beam_decode(**inputs, start_id=START_ID, end_id=END_ID, max_seq_len=T, top_k=TOP_K, beam_width=W)

        tokens, lengths, logprobs = (t.cpu() for t in device())
        want_tokens, want_scores = host_beam_loop(module, inputs, W)
        differ = [b for b in range(B)
                  if [tokens[b, p, :lengths[b, p]].tolist() for p in range(W)] != want_tokens[b]]
        agree = [b for b in range(B) if b not in differ]
        drift = float((logprobs.double() - torch.tensor(want_scores, dtype=torch.float64))[agree].abs().max()) if agree else None
        before = ops.launch_counts(aggregation=True, sequence=True, decode=True, beam=True)
        device()
        launches = {k: v / T for k, v in ops.launches_since(before).items()}   # plan builds: once per call, not per step
        for _ in range(5):
            device()
            greedy()
        host_beam_loop(module, inputs, W)
        dev, gre, host = [], [], []
        for _ in range(rounds):
            dev.append(per_call_us(device, 10))
            gre.append(per_call_us(greedy, 10))
            host.append(per_call_us(lambda: host_beam_loop(module, inputs, W), 2))
        res["widths"][str(W)] = {
            "results": {"tokens": int(lengths.sum()), "finished": int((lengths < T).sum()),
                        "outside_vocabulary": int((tokens >= V).sum()), "samples_differing_from_host_route": len(differ),
                        "max_score_difference_where_equal": drift},
            "device_route": summary(dev), "greedy_decode_same_process": summary(gre), "host_route": summary(host),
            "device_over_greedy": round(statistics.median(dev) / statistics.median(gre), 2),
            "host_over_device": round(statistics.median(host) / statistics.median(dev), 2),
            "launches_per_step_device_route": launches}
        print(json.dumps({str(W): res["widths"][str(W)]}), flush=True)
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    main(ap.parse_args().out)
