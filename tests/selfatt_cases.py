"""Case specs of the MultiHeadSelfAttentionMessagePassing fixtures: tests/golden/make_golden_selfatt.py builds them from
the reference's class, tests/test_selfatt_cpu.py and tests/test_gpu_selfatt.py from
ptgnn_amd.layers.MultiHeadSelfAttentionMessagePassing.

A fixture is the arrays of `name.npz` plus those of its continuation files `name.pK.npz`: the float64 copies of a
1 076-node, 64-wide case do not fit one file of the size a committed file may have, so the generator fills a file up
to PART_BYTES of array data and goes on in the next one; `load` reads them back as one dict."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 900_000
INTERMEDIATE = 24      # intermediate_dimension of every case: not a multiple of 32, small next to the attention


def sizes(max_num_nodes):
    """Nodes per graph: a full window, a one-row graph, an empty graph, a one-row last window, three windows, a two-row
    graph and a tile-sized graph."""
    m = max_num_nodes
    return [m, 1, 0, m + 1, 2 * m + 7, 2, 65]


# (D, dk, dv, heads, max_num_nodes); `scale` multiplies x (6: peaked softmax rows); `unsorted`: the node -> graph map is
# shuffled (only its counts may matter); `target`: reference ids that are a permutation of all nodes
CASES = [
    ("selfatt_d32_k6v10h3", dict(D=32, dk=6, dv=10, heads=3, max=40, scale=1.0, unsorted=True, target=False, seed=31)),
    ("selfatt_d64_k32h8", dict(D=64, dk=32, dv=32, heads=8, max=40, scale=1.0, unsorted=False, target=False, seed=32)),
    ("selfatt_d64_k64h2_w250", dict(D=64, dk=64, dv=64, heads=2, max=250, scale=1.0, unsorted=True, target=False,
                                    seed=33)),
    ("selfatt_d32_k8h4_peaked", dict(D=32, dk=8, dv=8, heads=4, max=40, scale=6.0, unsorted=False, target=False,
                                     seed=34)),
    ("selfatt_d32_k8h4_target", dict(D=32, dk=8, dv=8, heads=4, max=40, scale=1.0, unsorted=True, target=True, seed=35)),
]
TARGET = "supernodes"
PREFIX = "_MultiHeadSelfAttentionMessagePassing__"
STATE_KEYS = [PREFIX + k for k in (
    "selfatt_head_transforms.weight", "summarization_layer.weight", "intermediate_layer.weight",
    "intermediate_layer.bias", "output_layer.weight", "output_layer.bias", "layer_norm1.weight", "layer_norm1.bias",
    "layer_norm2.weight", "layer_norm2.bias")]


def build(spec, ns, **overrides):
    """The layer of `spec` from the namespace `ns` (a module holding MultiHeadSelfAttentionMessagePassing)."""
    kw = dict(input_state_dimension=spec["D"], key_query_dimension=spec["dk"], value_dimension=spec["dv"],
              output_dimension=spec["D"], intermediate_dimension=INTERMEDIATE, num_heads=spec["heads"], dropout_rate=0.0,
              target_reference=TARGET if spec["target"] else "all", max_num_nodes=spec["max"])
    kw.update(overrides)
    return ns.MultiHeadSelfAttentionMessagePassing(**kw)


def differentiable_reference(ref_module):
    """Bind the name `torch` of the reference's selfattmessagepassing module to a stand-in whose `no_grad()` does
    nothing.  Its window generator yields inside `with torch.no_grad()`, which leaves autograd switched off for the
    attention of lines 105-115; with the stand-in, torch differentiates the reference's own operator sequence."""
    import contextlib

    import torch

    class _Torch:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def no_grad():
            return contextlib.nullcontext()

    ref_module.torch = _Torch()


def files(name):
    return [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".p[0-9].npz")))


def load(name):
    out = {}
    for path in files(name):
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    return out


def call(layer, spec, x, fx_index, fx_ids=None, to=lambda t: t):
    """forward of `layer` on the fixture's inputs: the index is `node_to_graph_idx` of an "all" case and
    reference_node_graph_idx[TARGET] of a target case (whose node_to_graph_idx is unused)."""
    import torch
    idx = to(torch.as_tensor(fx_index))
    if not spec["target"]:
        return layer(x, [], idx, {}, {}, [])
    ids = to(torch.as_tensor(fx_ids))
    return layer(x, [], to(torch.zeros(x.shape[0], dtype=torch.int64)), {TARGET: ids}, {TARGET: idx}, [])
