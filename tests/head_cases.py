"""Cases of the task-head fixtures: tests/golden/make_golden_heads.py builds the heads from the reference's classes,
tests/test_heads_cpu.py and tests/test_gpu_heads.py from ptgnn_amd.heads -- both around `StubGnn`, a module with
`output_node_state_dim` whose call returns a `GnnOutput` holding the node states it is given.

Every case has two minibatches (the fixture's plain keys and its `second.` keys: other node states and targets, the same
index tensors), so that the metrics after two calls are not the metrics after one.  Input conditions (asserted by the
generator and by tests/test_heads_cpu.py on the reference's own numbers): every PPI logit has |l| >= 1e-4, the top two
logits of every Graph2Class row and the top two scores of every VarMisuse slot differ by >= 1e-3 -- under these, counts
and arg-maxes are compared exactly.  The seeds were chosen so that the conditions hold."""
import glob
import os

import numpy as np
import torch
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

G2C_CASES = [
    ("heads_g2c_small", dict(D=12, C=3, S=1, N=9, seed=31)),
    ("heads_g2c_wide", dict(D=64, C=100, S=37, N=150, seed=32)),
    ("heads_g2c_mixed", dict(D=12, C=100, S=37, N=60, seed=33)),
    ("heads_g2c_repeat", dict(D=64, C=3, S=37, N=20, repeat=True, seed=34)),      # a supernode id taken more than once
]
VM_CASES = [
    ("heads_vm_small", dict(H=8, sizes=[3], N=12, seed=41)),
    ("heads_vm_batch", dict(H=64, sizes=[1, 4, 2, 9, 3], N=80, seed=42)),
    ("heads_vm_shuffled", dict(H=8, sizes=[1, 4, 2, 9, 3], N=40, shuffle=True, seed=43)),   # a slot's candidates not contiguous
    ("heads_vm_one_slot", dict(H=64, sizes=[7], N=30, seed=44)),
]
PPI_CASES = [
    ("heads_ppi_single", dict(D=12, C=1, N=1, seed=51)),
    # 2 x 24 200 logits: node states of scale 8 spread them enough that some seed keeps every one away from 0
    ("heads_ppi_wide", dict(D=64, C=121, N=200, scale=8.0, seed=52)),
    ("heads_ppi_one_class", dict(D=64, C=1, N=200, seed=53)),
    ("heads_ppi_one_node", dict(D=12, C=121, N=1, seed=54)),
]
LFE_CASES = [
    ("heads_lfe_none", dict(F=50, D=64, N=33, act=None, seed=61)),
    ("heads_lfe_tanh", dict(F=50, D=64, N=33, act="tanh", seed=62)),
]
KINDS = {"g2c": G2C_CASES, "vm": VM_CASES, "ppi": PPI_CASES}
ALL_HEAD_CASES = [(kind, name, spec) for kind, cases in KINDS.items() for name, spec in cases]


class StubGnn(nn.Module):
    """Stands where the GNN stands: `output_cls` is the GnnOutput class of whoever builds the head."""

    def __init__(self, dim: int, output_cls):
        super().__init__()
        self.output_node_state_dim = dim
        self._output_cls = output_cls

    def forward(self, *, node_states, references, reference_graphs, num_graphs):
        node_to_graph = torch.zeros(node_states.shape[0], dtype=torch.int64, device=node_states.device)
        return self._output_cls(node_states, node_states, node_to_graph, references, reference_graphs, num_graphs)


def state_dim(kind, spec):
    return spec["H"] if kind == "vm" else spec["D"]


def build(kind, spec, ns, output_cls):
    """The head of `spec` from the namespace `ns` (holding the three classes) around a StubGnn."""
    gnn = StubGnn(state_dim(kind, spec), output_cls)
    if kind == "g2c":
        return ns.Graph2ClassModule(gnn, spec["C"])
    if kind == "vm":
        return ns.VarMisuseGraphModel(gnn)
    return ns.PPIClassification(gnn, spec["C"])


def make_inputs(kind, spec, gen):
    """{name: CPU tensor} for the two minibatches of a case (`second.` prefix for the second one's states / targets)."""
    N, dim = spec["N"], state_dim(kind, spec)
    scale = spec.get("scale", 1.0)
    out = {"node_states": scale * torch.randn(N, dim, generator=gen),
           "second.node_states": scale * torch.randn(N, dim, generator=gen)}
    if kind == "g2c":
        S, C = spec["S"], spec["C"]
        idx = torch.randint(0, N, (S,), generator=gen)
        if spec.get("repeat"):
            idx[1] = idx[0]
            idx[S - 1] = idx[0]
        out["supernodes"] = idx
        out["supernode_graphs"] = torch.arange(S)
        for key in ("targets", "second.targets"):
            t = torch.randint(0, C, (S,), generator=gen)
            t[0] = C - 1
            t[S - 1] = 0
            out[key] = t
    elif kind == "vm":
        sizes = spec["sizes"]
        G, Cn = len(sizes), sum(sizes)
        cand_slot = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
        if spec.get("shuffle"):
            cand_slot = cand_slot[torch.randperm(Cn, generator=gen)]
        out["candidate_nodes"] = torch.randperm(N, generator=gen)[:Cn]      # distinct: equal nodes of a slot would tie
        out["candidate_slots"] = cand_slot
        out["slot_nodes"] = torch.randint(0, N, (G,), generator=gen)
        for key in ("targets", "second.targets"):       # per slot the position of one of ITS candidates
            picks = []
            for g in range(G):
                own = torch.nonzero(cand_slot == g).flatten()
                picks.append(int(own[int(torch.randint(0, own.shape[0], (1,), generator=gen))]))
            out[key] = torch.tensor(picks, dtype=torch.int64)
    else:
        for key in ("targets", "second.targets"):
            out[key] = torch.rand(N, spec["C"], generator=gen) < 0.3
    return out


def call_args(kind, inputs, second=False, to=lambda t: t, states=None):
    """The positional arguments of the head's forward for one of the two minibatches; `states` replaces the node states
    (a leaf that requires grad)."""
    pre = "second." if second else ""
    x = to(inputs[pre + "node_states"]) if states is None else states
    targets = to(inputs[pre + "targets"])
    if kind == "g2c":
        data = dict(node_states=x, references={"supernodes": to(inputs["supernodes"])},
                    reference_graphs={"supernodes": to(inputs["supernode_graphs"])}, num_graphs=inputs["supernodes"].shape[0])
        return data, targets, None
    if kind == "vm":
        data = dict(node_states=x,
                    references={"candidate_nodes": to(inputs["candidate_nodes"]), "slot_node_idx": to(inputs["slot_nodes"])},
                    reference_graphs={"candidate_nodes": to(inputs["candidate_slots"])},
                    num_graphs=inputs["slot_nodes"].shape[0])
        return data, targets
    return dict(node_states=x, references={}, reference_graphs={}, num_graphs=1), targets


def build_lfe(spec, ns):
    return ns.LinearFeatureEmbedder(spec["F"], spec["D"], nn.Tanh() if spec["act"] == "tanh" else None)


def files(name):
    return [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".p*.npz")))


def load(name):
    out = {}
    for path in files(name):
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    return out


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


INPUT_KEYS = ("node_states", "second.node_states", "targets", "second.targets", "supernodes", "supernode_graphs",
              "candidate_nodes", "candidate_slots", "slot_nodes")


def inputs_of(fx):
    return {k: torch.from_numpy(fx[k]) for k in INPUT_KEYS if k in fx}


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own numbers the input conditions are about, from a fixture's inputs and initial parameters (float64)
# ---------------------------------------------------------------------------------------------------------------------
def _param(fx, suffix):
    (key,) = [k for k in fx if k.startswith("state.") and k.endswith(suffix)]
    return torch.from_numpy(fx[key]).double()


def reference_logits(kind, fx, second=False):
    """float64 logits [R, C] (g2c, ppi) or candidate scores [Cn] (vm) of one minibatch of a fixture."""
    x = torch.from_numpy(fx[("second." if second else "") + "node_states"]).double()
    if kind == "g2c":
        return x[torch.from_numpy(fx["supernodes"])] @ _param(fx, "node_to_class.weight").t() + _param(fx, "node_to_class.bias")
    if kind == "ppi":
        return x @ _param(fx, "to_logits.weight").t() + _param(fx, "to_logits.bias")
    w = _param(fx, "candidate_scores.weight")
    cand = x[torch.from_numpy(fx["candidate_nodes"])]
    slot = x[torch.from_numpy(fx["slot_nodes"])][torch.from_numpy(fx["candidate_slots"])]
    return (torch.cat((cand, slot), dim=-1) @ w.t()).squeeze(-1)


def conditions_hold(kind, fx):
    """The input conditions of a fixture, on both of its minibatches."""
    for second in (False, True):
        v = reference_logits(kind, fx, second)
        if kind == "ppi":
            if float(v.abs().min()) < 1e-4:
                return False
        elif kind == "g2c":
            if v.shape[1] > 1 and float((v.topk(2, dim=-1)[0][:, 0] - v.topk(2, dim=-1)[0][:, 1]).min()) < 1e-3:
                return False
        else:
            slots = torch.from_numpy(fx["candidate_slots"])
            for g in range(int(slots.max()) + 1):
                own = v[slots == g]
                if own.shape[0] > 1 and float(own.topk(2)[0][0] - own.topk(2)[0][1]) < 1e-3:
                    return False
    return True
