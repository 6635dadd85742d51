"""Cases of the Graph2SeqModule fixtures: tests/golden/make_golden_graph2seq.py builds the module from the reference's
classes, tests/test_graph2seq_cpu.py and tests/test_gpu_vocab_loss.py from ptgnn_amd -- both around `StubGnn`, a module
with `input_node_state_dim` / `output_node_state_dim` whose call returns a `GnnOutput` holding the node states it is given,
the MultiheadSelfAttentionVarSizedElementReduce summariser over SimpleVarSizedElementReduce("max") that
graph2seq.py:116-122 builds, and GruCopyingDecoder.

A case is D_in / D_out (input / output node state widths; the decoder's H = Dm = D_out), the summariser's heads, V, E, B
graphs, T tokens per target, the backbone nodes per graph (`sizes`) and the nodes per graph (`nodes`).  The decoder side
(backbone -> graph map, tokens, copyable entries, lengths) is `decoder_cases.make_inputs`, so every case has its
conditions: a shuffled backbone map with a graph without backbone nodes in the middle and the last graph with some, an UNK
target with and one without a valid copy, locations with nothing to copy, lengths shorter than L.  A backbone entry is any
node of its graph, so nodes repeat.  Every case has two minibatches (the fixture's plain keys and its `second.` keys: other
node states, the same index tensors and decoder data)."""
import re

import numpy as np
import torch
from torch import nn

import decoder_cases
from decoder_cases import UNK_ID, files, state_of  # noqa: F401  (the fixture file layout is the decoder's)

CASES = [
    ("graph2seq_small", dict(D_in=8, D_out=12, heads=4, V=50, E=12, B=4, T=6, sizes=[150, 1, 0, 9],
                             nodes=[160, 3, 2, 12], seed=71)),
    ("graph2seq_odd", dict(D_in=5, D_out=7, heads=3, V=23, E=10, B=3, T=4, sizes=[130, 0, 5], nodes=[131, 2, 9],
                           seed=72)),                                                    # widths not multiples of 4
    ("graph2seq_wide", dict(D_in=64, D_out=128, heads=8, V=300, E=32, B=5, T=8, sizes=[129, 1, 0, 57, 9],
                            nodes=[135, 3, 2, 60, 12], seed=73)),
]
DECODER_KEYS = ("target_token_ids", "copyable_elements_idxs", "copyable_elements_sample_idxs", "target_lengths")
ENCODER_KEYS = ("input_states", "output_states", "node_to_graph", "backbone_nodes", "backbone_graphs")
INPUT_KEYS = ENCODER_KEYS + ("second.input_states", "second.output_states") + DECODER_KEYS


class StubGnn(nn.Module):
    """Stands where the GNN stands: `output_cls` is the GnnOutput class of whoever builds the module."""

    def __init__(self, d_in: int, d_out: int, output_cls):
        super().__init__()
        self.input_node_state_dim, self.output_node_state_dim = d_in, d_out
        self._output_cls = output_cls

    def forward(self, *, input_states, output_states, node_to_graph, backbone_nodes, backbone_graphs, num_graphs):
        return self._output_cls(input_states, output_states, node_to_graph, {"backbone_nodes": backbone_nodes},
                                {"backbone_nodes": backbone_graphs}, num_graphs)


def build(spec, ns, output_cls, dropout_rate=0.0):
    """The module of `spec` from the namespace `ns` (holding Graph2SeqModule, GruCopyingDecoder,
    MultiheadSelfAttentionVarSizedElementReduce and SimpleVarSizedElementReduce): decoder first, then the summariser."""
    d_in, d_out = spec["D_in"], spec["D_out"]
    decoder = ns.GruCopyingDecoder(vocabulary_size=spec["V"], embedding_size=spec["E"], hidden_size=d_out,
                                   memories_hidden_dim=d_out, unk_id=UNK_ID, dropout_rate=dropout_rate)
    summariser = ns.MultiheadSelfAttentionVarSizedElementReduce(
        input_representation_size=d_in + d_out, hidden_size=d_in + d_out, output_representation_size=d_out,
        num_heads=spec["heads"], query_representation_summarizer=ns.SimpleVarSizedElementReduce("max"))
    return ns.Graph2SeqModule(StubGnn(d_in, d_out, output_cls), decoder, summariser)


def make_inputs(spec, gen):
    """{name: CPU tensor} for the two minibatches of a case."""
    decoder = decoder_cases.make_inputs(dict(spec, H=spec["D_out"], Dm=spec["D_out"]), gen)
    graphs = decoder["input_memories_origin_idx"]                          # graph of every backbone entry, shuffled
    nodes = torch.tensor(spec["nodes"])
    first = torch.cumsum(nodes, 0) - nodes
    pick = torch.minimum((torch.rand(graphs.shape[0], generator=gen) * nodes[graphs]).long(), nodes[graphs] - 1)
    N = int(nodes.sum())
    out = {"node_to_graph": torch.repeat_interleave(torch.arange(spec["B"]), nodes),
           "backbone_nodes": first[graphs] + pick, "backbone_graphs": graphs}
    for pre in ("", "second."):
        out[pre + "input_states"] = torch.randn(N, spec["D_in"], generator=gen)
        out[pre + "output_states"] = torch.randn(N, spec["D_out"], generator=gen)
    out.update({k: decoder[k] for k in DECODER_KEYS})
    return out


def call_args(spec, inputs, second=False, to=lambda t: t, states=None):
    """The keyword arguments of the module's forward for one of the two minibatches; `states` = (input, output) node
    states that replace the minibatch's own (leaves that require grad)."""
    pre = "second." if second else ""
    x_in, x_out = states if states is not None else (to(inputs[pre + "input_states"]), to(inputs[pre + "output_states"]))
    encoder = dict(input_states=x_in, output_states=x_out, node_to_graph=to(inputs["node_to_graph"]),
                   backbone_nodes=to(inputs["backbone_nodes"]), backbone_graphs=to(inputs["backbone_graphs"]),
                   num_graphs=spec["B"])
    return dict(encoder_mb_data=encoder, decoder_mb_data={k: to(inputs[k]) for k in DECODER_KEYS})


PIECE_BYTES = 300_000      # an array past this is stored as row blocks `key#0`, `key#1`, ... (the summariser's output
#                            layer of the wide case alone is 786 432 bytes: more than a fixture file may hold)


def pieces(key, array):
    """[(stored key, array)] of one array of a fixture."""
    if array.nbytes <= PIECE_BYTES or array.ndim == 0:
        return [(key, array)]
    rows = max(1, PIECE_BYTES // max(1, array.nbytes // array.shape[0]))
    return [(f"{key}#{i}", array[at:at + rows]) for i, at in enumerate(range(0, array.shape[0], rows))]


def load(name):
    """A fixture and its continuation files as one dict of arrays, the row blocks of a large array joined again."""
    stored = decoder_cases.load(name)
    out, blocks = {}, {}
    for key, v in stored.items():
        m = re.fullmatch(r"(.*)#(\d+)", key)
        if m:
            blocks.setdefault(m.group(1), {})[int(m.group(2))] = v
        else:
            out[key] = v
    for key, parts in blocks.items():
        out[key] = np.concatenate([parts[i] for i in range(len(parts))], axis=0)
    return out


def inputs_of(fx):
    return {k: torch.from_numpy(fx[k]) for k in INPUT_KEYS}


def conditions_hold(spec, inputs):
    """The input conditions of the module docstring, on the inputs of a case."""
    graphs, nodes, B, L = inputs["backbone_graphs"], inputs["backbone_nodes"], spec["B"], spec["T"] - 1
    counts = torch.bincount(graphs, minlength=B)
    tokens, locations = inputs["target_token_ids"], inputs["copyable_elements_sample_idxs"]
    has_copy = torch.bincount(locations, minlength=B * L).reshape(B, L) > 0
    unk = tokens[:, 1:] == UNK_ID
    return bool((counts[1:-1] == 0).any() and counts[-1] > 0 and not torch.equal(graphs, graphs.sort()[0])
                and torch.equal(inputs["node_to_graph"][nodes], graphs) and nodes.unique().shape[0] < nodes.shape[0]
                and (unk & has_copy).any() and (unk & ~has_copy).any() and (~has_copy).any()
                and (L == 1 or (inputs["target_lengths"] < L).any()))
