"""Graph2Seq decoder timings (GruCopyingDecoder at the reference's defaults: L = 7 steps, H = Dm = 128, E = 256,
V = 20 000; B = 64 samples with a few hundred memories each).  Not part of bench.py.

    python scripts/decoder_bench.py [--out FILE] [--reps N]

HIP events, median of --reps after warm-up:
  * the fused copy scores (ops.segment_scores) and their rate on the algorithmic bytes I*K*4 + I*L*4 + G*L*(K+1)*4
    (+ perm), and the backward (ops.segment_scores_backward) on 2*I*K*4 + 2*I*L*4 + 2*G*L*(K+1)*4 (+ perm);
  * `_compute_logprobs` without gradients and a training step (`forward` + backward w.r.t. the memories, the initial
    states and every weight), dropout 0 and dropout 0.2, against the reference's operator sequence
    (grucopydecoder.py:70-212) on the same GPU over the torch_scatter facade with torch's nn.GRU / nn.Linear / einsum,
    i.e. what running the reference class after `ptgnn_amd.scatter.install()` does.
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/decoder_bench.py`."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ptgnn_amd import ops, scatter as S, sequence  # noqa: E402
from ptgnn_amd.layers import _index_plan  # noqa: E402

PEAK_TBPS = 8.0
V, E, H, DM, B, T, UNK = 20_000, 256, 128, 128, 64, 8, 1
L = T - 1
P = "_GruCopyingDecoder__"


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


def facade_logprobs(m, initial_states, x, idx, token_ids):
    """grucopydecoder.py:70-142 line by line, torch_scatter = ptgnn_amd.scatter (HIP), everything else torch."""
    sub = dict(m.named_children())
    emb, gru, drop = sub[P + "embedding_layer"], sub[P + "output_gru"], sub[P + "dropout"]
    std_l, copy_l = sub[P + "memories_to_standard_attention"], sub[P + "memories_to_copy_attention"]
    par = dict(m.named_parameters())
    o, state = gru(drop(emb(token_ids)), initial_states.unsqueeze(0))
    o = o.contiguous()
    std, cp = std_l(x), drop(copy_l(x))
    per_input = o[idx]
    std_scores = torch.einsum("ilh,ih->il", per_input, std)
    copy_scores = torch.einsum("ilh,ih->il", per_input, cp)
    logp = S.scatter_log_softmax(std_scores, index=idx, dim=0, eps=0)
    mul = torch.einsum("il,ih->ilh", torch.exp(logp), std)
    out = S.scatter_add(mul, index=idx, dim=0, dim_size=o.shape[0])
    target = torch.einsum("blh,hd,vd->blv", torch.cat((drop(out), o), dim=-1), par[P + "hidden_to_vocab"],
                          drop(emb.weight)) + par[P + "vocab_bias"]
    total = S.scatter_logsumexp(copy_scores, index=idx, dim=0, dim_size=o.shape[0], eps=0)
    norm = torch.logsumexp(torch.cat((target, total.unsqueeze(-1)), dim=-1), dim=-1)
    return copy_scores - norm[idx], target - norm.unsqueeze(-1), state


def facade_loss(m, inp):
    """grucopydecoder.py:166-212 over `facade_logprobs`."""
    tokens, where = inp["target_token_ids"], inp["copyable_elements_sample_idxs"]
    copy_lp, target_lp, _ = facade_logprobs(m, inp["initial_states"], inp["input_memories"],
                                            inp["input_memories_origin_idx"], tokens[:, :-1])
    n = tokens.shape[0] * L
    valid = S.scatter_add(torch.ones_like(where), index=where, dim=0, dim_size=n).reshape(-1, L) > 0
    gen = torch.gather(target_lp, index=tokens[:, 1:].unsqueeze(-1), dim=-1).squeeze(-1)
    gen = gen.masked_fill(valid & (tokens[:, 1:] == UNK), -math.inf)
    cop = S.scatter_logsumexp(copy_lp.flatten()[inp["copyable_elements_idxs"]], index=where, dim=0, dim_size=n,
                              eps=0).view(-1, L)
    any_ok = torch.logsumexp(torch.stack((gen, cop)), dim=0)
    mask = (torch.arange(L, device=any_ok.device).unsqueeze(0) < inp["target_lengths"].unsqueeze(1)).float()
    return -((any_ok * mask).sum(-1) / mask.sum(-1)).mean()


def batch(seed):
    g = torch.Generator().manual_seed(seed)
    sizes = (torch.rand(B, generator=g) * 400 + 100).long()                  # 100 .. 500 memories per sample
    idx = torch.repeat_interleave(torch.arange(B), sizes)
    idx = idx[torch.randperm(idx.shape[0], generator=g)]
    n = idx.shape[0]
    tokens = torch.randint(2, V, (B, T), generator=g)
    memory = torch.randint(0, n, (4 * B,), generator=g)                       # four copyable memories per sample
    step = torch.randint(0, L, (4 * B,), generator=g)
    inp = dict(input_memories=torch.randn(n, DM, generator=g), input_memories_origin_idx=idx,
               initial_states=torch.randn(B, H, generator=g), target_token_ids=tokens,
               copyable_elements_idxs=memory * L + step, copyable_elements_sample_idxs=idx[memory] * L + step,
               target_lengths=torch.randint(2, L + 1, (B,), generator=g))
    return {k: v.cuda() for k, v in inp.items()}


def run(dropout, reps):
    torch.manual_seed(1)
    m = sequence.GruCopyingDecoder(V, E, H, DM, UNK, dropout).cuda()
    inp = batch(7)
    x, idx = inp["input_memories"], inp["input_memories_origin_idx"]
    n = x.shape[0]
    res = {"dropout": dropout, "I": n, "B": B, "L": L, "H": H, "Dm": DM, "E": E, "V": V}
    args = (inp["initial_states"], x, idx, inp["target_token_ids"][:, :-1])
    m.eval()
    with torch.no_grad():
        got, want = m._compute_logprobs(*args), facade_logprobs(m, *args)
        res["max_abs_vs_facade"] = max(float((a - b).abs().max()) for a, b in zip(got, want))
        res["infer_ms"] = t_med(lambda: m._compute_logprobs(*args), reps)
        res["infer_facade_ms"] = t_med(lambda: facade_logprobs(m, *args), reps)
        if dropout == 0.0:
            plan = _index_plan(idx, B)
            v = torch.randn(B, L, DM, device=x.device) / math.sqrt(DM)
            scores, lse = ops.segment_scores(x, v, plan)
            fwd = 4.0 * (n * DM + n * L + B * L * (DM + 1)) + 4.0 * n
            res["scores_ms"] = t_med(lambda: ops.segment_scores(x, v, plan), reps)
            res["scores_bytes"], res["scores_tbps"] = fwd, fwd / (res["scores_ms"] * 1e-3) / 1e12
            res["scores_frac_of_peak"] = res["scores_tbps"] / PEAK_TBPS
            gs, gl = torch.randn_like(scores), torch.randn_like(lse)
            bwd = 4.0 * (2 * n * DM + 2 * n * L + 2 * B * L * (DM + 1)) + 4.0 * n
            res["scores_backward_ms"] = t_med(lambda: ops.segment_scores_backward(x, v, plan, scores, lse, gs, gl), reps)
            res["scores_backward_bytes"] = bwd
            res["scores_backward_tbps"] = bwd / (res["scores_backward_ms"] * 1e-3) / 1e12
    m.train()
    live = dict(inp, input_memories=x.clone().requires_grad_(True),
                initial_states=inp["initial_states"].clone().requires_grad_(True))

    def step_ours():
        m.zero_grad(set_to_none=True)
        m(**live).backward()

    def step_facade():
        m.zero_grad(set_to_none=True)
        facade_loss(m, live).backward()

    res["train_step_ms"] = t_med(step_ours, reps)
    res["train_step_facade_ms"] = t_med(step_facade, reps)
    res["infer_speedup"] = res["infer_facade_ms"] / res["infer_ms"]
    res["train_speedup"] = res["train_step_facade_ms"] / res["train_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    out = {"reps": args.reps, "runs": [run(0.0, args.reps), run(0.2, args.reps)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
