"""Forward + backward of the three task heads alone (the GNN replaced by a module that hands back fixed node states which
require grad) at stand-ins for the cfg3 / cfg4 / cfg1 shapes, next to the torch composition of the same head, with the
C-ABI launch counters of one step.  20 warm-up steps, then 7 blocks of 50 steps, each closed by a device synchronise;
median / min / max of the blocks' per-step wall time.  The record behind profiles/heads_notes.md:

    python -m benchmarks.heads [--out profiles/heads_bench.json]
"""
import argparse
import json
import statistics
import time

import torch
from torch import nn

from ptgnn_amd import heads, ops
from ptgnn_amd.gnn import GnnOutput

DEV = torch.device("cuda")
F = torch.nn.functional


class StubGnn(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.output_node_state_dim = dim

    def forward(self, *, node_states, references, reference_graphs, num_graphs):
        node_to_graph = torch.zeros(node_states.shape[0], dtype=torch.int64, device=node_states.device)
        return GnnOutput(node_states, node_states, node_to_graph, references, reference_graphs, num_graphs)


def timed(fn, warm=20, blocks=7, per=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(per):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / per * 1e6)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def counts(fn):
    before = ops.launch_counts(aggregation=True, heads=True)
    fn()
    return ops.launches_since(before)


def segment_lse(scores, index, n):
    top = torch.full((n,), -float("inf"), device=scores.device).scatter_reduce(0, index, scores.detach(), "amax")
    total = torch.zeros(n, device=scores.device).index_add(0, index, (scores - top[index]).exp())
    return total.log() + top


def main(out=None):
    res = {}
    gen = torch.Generator().manual_seed(0)
    # cfg3: 48 graphs x ~2400 nodes, hidden 128 -> 100 classes, 50 supernodes per graph
    N, D, C, S = 116_000, 128, 100, 2400
    x = torch.randn(N, D, generator=gen).to(DEV).requires_grad_(True)
    idx = torch.randint(0, N, (S,), generator=gen).to(DEV)
    tgt = torch.randint(0, C, (S,), generator=gen).to(DEV)
    mod = heads.Graph2ClassModule(StubGnn(D), C).to(DEV)
    lin = torch.nn.Linear(D, C).to(DEV)
    data = dict(node_states=x, references={"supernodes": idx}, reference_graphs={"supernodes": idx}, num_graphs=48)
    def ours(): x.grad = None; mod(data, tgt, None).backward()
    def theirs(): x.grad = None; F.cross_entropy(lin(x[idx]), tgt).backward()
    res["cfg3_graph2class"] = dict(shape=f"N={N} D={D} C={C} S={S}", launches=counts(ours), ptgnn_amd=timed(ours), torch=timed(theirs))

    # cfg4: VarMisuse, hidden 64, 48 slots x 12 candidates
    N, H, G, K = 116_000, 64, 48, 12
    x4 = torch.randn(N, H, generator=gen).to(DEV).requires_grad_(True)
    cand = torch.randint(0, N, (G * K,), generator=gen).to(DEV)
    slot = torch.randint(0, N, (G,), generator=gen).to(DEV)
    cslot = torch.arange(G).repeat_interleave(K).to(DEV)
    corr = (torch.arange(G) * K + 3).to(DEV)
    vm = heads.VarMisuseGraphModel(StubGnn(H)).to(DEV)
    lin4 = torch.nn.Linear(2 * H, 1, bias=False).to(DEV)
    d4 = dict(node_states=x4, references={"candidate_nodes": cand, "slot_node_idx": slot}, reference_graphs={"candidate_nodes": cslot}, num_graphs=G)
    acc = [0]
    def ours4(): x4.grad = None; vm(d4, corr).backward()
    def theirs4():
        x4.grad = None
        sc = lin4(torch.cat((x4[cand], x4[slot][cslot]), dim=-1)).squeeze(-1)
        lp = sc - segment_lse(sc, cslot, G)[cslot]
        with torch.no_grad():
            best = torch.full((G,), -float("inf"), device=DEV).scatter_reduce(0, cslot, sc, "amax")
            acc[0] += int(((sc == best[cslot]) & (torch.arange(G * K, device=DEV) == corr[cslot])).sum())   # the reference's int(...)
        (-lp[corr].mean()).backward()
    res["cfg4_varmisuse"] = dict(shape=f"N={N} H={H} G={G} candidates={G * K}", launches=counts(ours4), ptgnn_amd=timed(ours4), torch=timed(theirs4))

    # cfg1: PPI, ~2400 nodes per minibatch, hidden 64 -> 121 labels
    N, D, C = 2400, 64, 121
    x1 = torch.randn(N, D, generator=gen).to(DEV).requires_grad_(True)
    t1 = (torch.rand(N, C, generator=gen) < 0.3).to(DEV)
    ppi = heads.PPIClassification(StubGnn(D), C).to(DEV)
    lin1 = torch.nn.Linear(D, C).to(DEV)
    d1 = dict(node_states=x1, references={}, reference_graphs={}, num_graphs=1)
    sums = [0.0, 0.0, 0.0]
    def ours1(): x1.grad = None; ppi(d1, t1).backward()
    def theirs1():
        x1.grad = None
        lg = lin1(x1)
        with torch.no_grad():
            p = torch.sigmoid(lg) >= 0.5
            tp, fp, fn = (p & t1).sum().float(), (p & ~t1).sum().float(), (~p & t1).sum().float()
            pr, re = tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)
            f1 = 2 * pr * re / (pr + re + 1e-10)
            sums[0] += float(f1.cpu()); sums[1] += float(pr.cpu()); sums[2] += float(re.cpu())               # the reference's reads
        F.binary_cross_entropy_with_logits(lg, t1.float(), reduction="none").sum(-1).mean().backward()
    res["cfg1_ppi"] = dict(shape=f"N={N} D={D} C={C}", launches=counts(ours1), ptgnn_amd=timed(ours1), torch=timed(theirs1))
    print(json.dumps(res, indent=1))
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    main(parser.parse_args().out)
