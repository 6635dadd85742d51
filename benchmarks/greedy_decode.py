"""One greedy-decoding call of GruCopyingDecoder at the reference's defaults (grucopydecoder.py:220-230 and the minibatches
of 50 of graph2seq.py:175-204): B = 50 samples, V = 20 000, max_seq_len = 8, H = 128, E = 256, about 200 memories per
sample -- on two routes, alternated in one process on the same seeded inputs:

  device    `GruCopyingDecoder.greedy_decode`: the loop on device tensors, one csrc/decode_step.hip launch per step;
  host      the reference's loop (grucopydecoder.py:375-457) restated here around `_compute_logprobs`, the only route
            before `greedy_decode` existed: `target_logprobs` [B, 1, V], torch.topk(100), three .cpu() copies, the Python
            dict merge per memory, the arg-max and the next token tensor built on the host.

The two routes' predictions are compared before timing and the comparison is part of the record (samples whose tokens
differ, largest log-probability difference; the weights are random, so a decision can sit closer than fp32 resolves).
5 warm-up calls per route, then 7 rounds of (10 device calls, 3 host calls), every call closed by a device synchronise (the host route ends in its
own read-backs); median / min / max of the rounds' per-call wall time, and the C-ABI launches of one step of the device
route.  The record behind profiles/greedy_decode_notes.md:

    python -m benchmarks.greedy_decode [--out profiles/greedy_decode_bench.json]
"""
import argparse
import json
import math
import statistics
import time

import numpy as np
import torch

from ptgnn_amd import ops, sequence

DEV = torch.device("cuda")
B, V, T, H, E, DM, PER_SAMPLE, TOP_K = 50, 20000, 8, 128, 256, 128, 200, 100
UNK_ID, START_ID, END_ID = 1, 2, 3


def make_case(seed=0):
    """The module (vocabulary scores spread so that vocabulary entries, copies and END all win somewhere) and the inputs:
    sizes around PER_SAMPLE, a shuffled memory -> sample map, element ids from 30 vocabulary ids and 10 outside keys per
    call -- so the memories of a sample fall into a few dozen value groups, as identifier tokens of one snippet do."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = sequence.GruCopyingDecoder(V, E, H, DM, UNK_ID, 0.2).eval()
    with torch.no_grad():
        state = module.state_dict()
        state[[k for k in state if k.endswith("hidden_to_vocab")][0]].mul_(5.0)
        state[[k for k in state if k.endswith("memories_to_copy_attention.weight")][0]].mul_(3.0)
        bias = state[[k for k in state if k.endswith("vocab_bias")][0]]
        bias.copy_(torch.randn(V, generator=g))
        bias[END_ID] += 4.0
    sizes = torch.randint(PER_SAMPLE // 2, PER_SAMPLE * 3 // 2 + 1, (B,), generator=g)
    index = torch.repeat_interleave(torch.arange(B), sizes)
    index = index[torch.randperm(index.shape[0], generator=g)]
    n = index.shape[0]
    pool = torch.randperm(V - 4, generator=g)[:30] + 4
    ids = torch.where(torch.rand(n, generator=g) < 0.6, pool[torch.randint(0, 30, (n,), generator=g)],
                      V + torch.randint(0, 10, (n,), generator=g))
    inputs = dict(input_memories=torch.randn(n, DM, generator=g), input_memories_origin_idx=index,
                  initial_states=torch.randn(B, H, generator=g), input_element_ids=ids)
    return module.to(DEV), {k: v.to(DEV) for k, v in inputs.items()}


def host_loop(module, inputs):
    """grucopydecoder.py:375-457 on extended ids (the dict is keyed by id instead of by string)."""
    x, index, h = inputs["input_memories"], inputs["input_memories_origin_idx"], inputs["initial_states"]
    values = inputs["input_element_ids"].cpu().tolist()
    feed = torch.tensor([[START_ID]] * B, device=DEV)
    tokens, logprobs, done = [[] for _ in range(B)], [0.0] * B, np.zeros(B, dtype=bool)
    with torch.no_grad():
        for _ in range(T):
            copy_logprobs, target_logprobs, state = module._compute_logprobs(h, x, index, feed)
            h = state.squeeze(0)
            top_logprobs, top_ids = torch.topk(target_logprobs.squeeze(1), min(TOP_K, V), dim=-1)
            top_logprobs, top_ids = top_logprobs.cpu().numpy(), top_ids.cpu().numpy()
            copy_logprobs = copy_logprobs.squeeze(1).cpu().numpy()
            predictions = [dict(zip(top_ids[b].tolist(), top_logprobs[b])) for b in range(B)]
            for b, value, c in zip(index.cpu().numpy(), values, copy_logprobs):
                predictions[b][value] = np.logaddexp(predictions[b].get(value, -math.inf), c)
            step = []
            for b in range(B):
                if done[b]:
                    step.append(END_ID)
                    continue
                predicted, value = max(predictions[b].items(), key=lambda kv: kv[1])
                if predicted == END_ID:
                    done[b] = True
                else:
                    tokens[b].append(predicted)
                step.append(predicted)
                logprobs[b] += float(value)
            feed = torch.tensor([[t if t < V else UNK_ID] for t in step], device=DEV)
    return tokens, logprobs


def device_call(module, inputs):
    return module.greedy_decode(**inputs, start_id=START_ID, end_id=END_ID, max_seq_len=T, top_k=TOP_K)


def per_call_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def summary(samples):
    return {"median_us": round(statistics.median(samples), 1), "min_us": round(min(samples), 1),
            "max_us": round(max(samples), 1)}


def main(out=None, rounds=7):
    module, inputs = make_case()
    tokens, lengths, logprobs = (t.cpu() for t in device_call(module, inputs))
    want_tokens, want_logprobs = host_loop(module, inputs)
    differ = [b for b in range(B) if tokens[b, :lengths[b]].tolist() != want_tokens[b]]
    agree = [b for b in range(B) if b not in differ]
    drift = float((logprobs.double() - torch.tensor(want_logprobs, dtype=torch.float64))[agree].abs().max())
    before = ops.launch_counts(aggregation=True, sequence=True, decode=True)
    device_call(module, inputs)
    launches = {k: v / T for k, v in ops.launches_since(before).items()}     # plan builds: once per call, not per step
    for _ in range(5):
        device_call(module, inputs)
        host_loop(module, inputs)
    device, host = [], []
    for _ in range(rounds):
        device.append(per_call_us(lambda: device_call(module, inputs), 10))
        host.append(per_call_us(lambda: host_loop(module, inputs), 3))
    res = {"shape": dict(B=B, V=V, max_seq_len=T, H=H, E=E, Dm=DM, memories=int(inputs["input_memories"].shape[0]),
                         top_k=TOP_K),
           "predictions": {"tokens": int(lengths.sum()), "ended": int((lengths < T).sum()),
                           "outside_vocabulary": int((tokens >= V).sum()), "samples_differing_from_host_route": len(differ),
                           "max_logprob_difference_where_equal": drift},
           "device_route": summary(device), "host_route": summary(host),
           "host_over_device": round(statistics.median(host) / statistics.median(device), 2),
           "launches_per_step_device_route": launches}
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
