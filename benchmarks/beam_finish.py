"""The finishing route of GruCopyingDecoder.beam_decode (back-pointers, the live count and its read-backs, the early
exit) against the default call, at the shapes of benchmarks/beam_decode.py: the same seeded module and inputs (B = 50,
V = 20 000, H = 128, E = 256, about 200 memories per sample), alternating rounds in one process, every call closed by a
device synchronise, median (min - max) of the rounds' per-call wall time.  Three legs:

  (a) where the feature cannot help: END is never chosen at this shape (profiles/beam_decode_notes.md), max_seq_len = 8,
      W = 1, 4, 8.  The default call against `early_exit=2` (back-pointers and read-backs, no exit) and against
      `early_exit=max_seq_len` (back-pointers alone: no count is sent that nobody would look at).  The default call of
      the PARENT commit is measured by this file run from a checkout of that commit (it uses no new keyword there):
          cd <parent checkout> && python <this file> --default-only 8 > before.json     (and again afterwards)
      in the same session on the same device, and `--parent-records before.json after.json` puts those records beside
      this process's rounds.
  (b) the exit: END's bias raised until every hypothesis has finished after a step s* near max_seq_len / 2 (s* is read off
      the lengths of a full run and printed), `early_exit` = 0, 1, 2, 4.
  (c) back-pointers where the copied histories are largest: max_seq_len = 32, W = 8, the default call against
      `early_exit=max_seq_len` and `early_exit=2`.

The results of the routes are compared bit for bit before timing; that is part of the record.  The record behind
profiles/beam_finish_notes.md:

    python -m benchmarks.beam_finish [--parent-records FILE ...] [--out profiles/beam_finish_bench.json]
"""
import argparse
import json
import os
import sys

import torch

WIDTHS = (1, 4, 8)
ROUNDS, CALLS, WARMUP = 7, 10, 5


def decode(module, inputs, W, T, **more):
    from benchmarks.greedy_decode import END_ID, START_ID, TOP_K
    return module.beam_decode(**inputs, start_id=START_ID, end_id=END_ID, max_seq_len=T, top_k=TOP_K, beam_width=W, **more)


def alternate(routes, rounds=ROUNDS, calls=CALLS):
    """{name: fn} -> {name: summary}: WARMUP calls each, then `rounds` rounds of `calls` calls of every route in turn."""
    from benchmarks.greedy_decode import per_call_us, summary
    for _ in range(WARMUP):
        for fn in routes.values():
            fn()
    samples = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            samples[name].append(per_call_us(fn, calls))
    return {name: summary(v) for name, v in samples.items()}


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def default_only(T):
    """The default call alone: what this file measures when it is run from a tree that may not have the new keywords."""
    from benchmarks.greedy_decode import make_case
    module, inputs = make_case()
    return {str(W): alternate({"default": lambda: decode(module, inputs, W, T)})["default"] for W in WIDTHS}


def leg_a(module, inputs, T, parent_records):
    from ptgnn_amd import ops
    out = {"parent_commit_default": [json.load(open(path)) for path in parent_records], "widths": {}}
    for W in WIDTHS:
        default = decode(module, inputs, W, T)
        assert same(default, decode(module, inputs, W, T, early_exit=2))
        assert same(default, decode(module, inputs, W, T, early_exit=T))
        before = ops.launch_counts(beam=True, beam_finish=True)
        decode(module, inputs, W, T, early_exit=2)
        launches = ops.launches_since(before)
        res = alternate({"default": lambda: decode(module, inputs, W, T),
                         "early_exit_2": lambda: decode(module, inputs, W, T, early_exit=2),
                         "early_exit_T": lambda: decode(module, inputs, W, T, early_exit=T)})
        res["finished_slots"] = int((default[1] < T).sum())
        res["launches_early_exit_2"] = launches
        res["early_exit_2_minus_default_us"] = round(res["early_exit_2"]["median_us"] - res["default"]["median_us"], 1)
        res["early_exit_T_minus_default_us"] = round(res["early_exit_T"]["median_us"] - res["default"]["median_us"], 1)
        res["default_spread_us"] = round(res["default"]["max_us"] - res["default"]["min_us"], 1)
        out["widths"][str(W)] = res
        print(json.dumps({"a": {str(W): res}}), flush=True)
    return out


def leg_b(T):
    """END's bias raised: the first raise, in steps of 1, at which every hypothesis of the W = 8 search has finished after a
    step s* <= T / 2."""
    from benchmarks.greedy_decode import END_ID, make_case
    from ptgnn_amd import ops
    module, inputs = make_case()
    bias = [v for k, v in module.state_dict().items() if k.endswith("vocab_bias")][0]
    out = {}
    for raised in range(0, 40):
        lengths = decode(module, inputs, max(WIDTHS), T)[1]
        if int(lengths.max()) <= T // 2:       # a hypothesis that finished at step s has s tokens
            break
        with torch.no_grad():
            bias[END_ID] += 1.0
    out["end_bias_raised_by"] = raised
    for W in WIDTHS:
        default = decode(module, inputs, W, T)
        s_star = int(default[1].max())
        res = {"s_star": s_star if s_star < T else None}
        routes = {"early_exit_0": lambda: decode(module, inputs, W, T)}
        for n in (1, 2, 4):
            assert same(default, decode(module, inputs, W, T, early_exit=n))
            before = ops.launch_counts(beam_finish=True)
            decode(module, inputs, W, T, early_exit=n)
            res[f"steps_issued_early_exit_{n}"] = ops.launches_since(before).get("beam_step_links")
            routes[f"early_exit_{n}"] = (lambda n: lambda: decode(module, inputs, W, T, early_exit=n))(n)
        res.update(alternate(routes))
        out[str(W)] = res
        print(json.dumps({"b": {str(W): res}}), flush=True)
    return out


def leg_c(module, inputs, T=32, W=8):
    default = decode(module, inputs, W, T)
    assert same(default, decode(module, inputs, W, T, early_exit=T))
    assert same(default, decode(module, inputs, W, T, early_exit=2))
    res = alternate({"default": lambda: decode(module, inputs, W, T),
                     "early_exit_T": lambda: decode(module, inputs, W, T, early_exit=T),
                     "early_exit_2": lambda: decode(module, inputs, W, T, early_exit=2)}, calls=4)
    res.update(max_seq_len=T, W=W, finished_slots=int((default[1] < T).sum()),
               copied_history_bytes_per_step=16 * T * int(default[1].numel()),
               back_pointer_bytes_per_step=8 * int(default[1].numel()))
    print(json.dumps({"c": res}), flush=True)
    return res


def main(out=None, parent_records=()):
    from benchmarks.greedy_decode import B, T, V, make_case
    module, inputs = make_case()
    res = {"shape": dict(B=B, V=V, max_seq_len=T, memories=int(inputs["input_memories"].shape[0])),
           "rounds": ROUNDS, "calls_per_round": CALLS,
           "a_no_exit_possible": leg_a(module, inputs, T, parent_records),
           "b_exit": leg_b(T),
           "c_back_pointers_long": leg_c(module, inputs)}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-records", nargs="*", default=(), metavar="FILE",
                    help="records of --default-only runs in a checkout of the parent commit")
    ap.add_argument("--default-only", type=int, default=None, metavar="T", help="the default call alone, as JSON")
    args = ap.parse_args()
    if args.default_only is not None:
        sys.path[0] = os.getcwd()              # the tree this process was started in, not the tree of this file
        print(json.dumps(default_only(args.default_only)))
    else:
        main(args.out, args.parent_records)
