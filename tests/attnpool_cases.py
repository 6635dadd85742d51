"""Module specs of the attention-pooling fixtures: tests/golden/make_golden_attnpool.py builds them from the reference's
classes, tests/test_attention_pool_cpu.py and tests/test_gpu_attention_pool.py from ptgnn_amd.reduceops.

`query` is "max" / "mean" (SimpleVarSizedElementReduce), "wsum" (WeightedSumVarSizedElementReduce(D)) -- all D wide, so
hidden = D -- or a nested attention spec whose output width is the outer hidden size (hidden != D)."""

# elements per sample: one beyond the 128-row chunk, a 1-element sample, an empty one in the middle; the fixtures pass
# num_samples = len(SIZES) + 1, so the last sample lies beyond the largest index and is empty too
SIZES = [150, 1, 0, 9, 20, 5]
NUM_SAMPLES = len(SIZES) + 1

CASES = [
    ("attnpool_single_max", dict(cls="single", D=8, hidden=8, out=6, query="max", seed=11)),
    ("attnpool_single_nested", dict(cls="single", D=8, hidden=12, out=5, seed=12,
                                    query=dict(cls="multi", D=8, hidden=8, out=12, heads=2, query="mean", value=False))),
    ("attnpool_mh1_max", dict(cls="multi", D=8, hidden=8, out=6, heads=1, query="max", value=False, seed=13)),
    ("attnpool_mh4_mean", dict(cls="multi", D=8, hidden=8, out=6, heads=4, query="mean", value=False, seed=14)),
    ("attnpool_mh8_wsum", dict(cls="multi", D=16, hidden=16, out=8, heads=8, query="wsum", value=False, seed=15)),
    ("attnpool_mh4_value_max", dict(cls="multi", D=8, hidden=8, out=6, heads=4, query="max", value=True, seed=16)),
    ("attnpool_mh8_value_wsum", dict(cls="multi", D=16, hidden=16, out=8, heads=8, query="wsum", value=True, seed=17)),
    ("attnpool_mh2_value_nested", dict(cls="multi", D=6, hidden=10, out=4, heads=2, value=True, seed=18,
                                       query=dict(cls="single", D=6, hidden=6, out=10, query="max"))),
]


def build(spec, ns):
    """The module of `spec` from the namespace `ns` (a module holding SimpleVarSizedElementReduce,
    WeightedSumVarSizedElementReduce, SelfAttentionVarSizedElementReduce, MultiheadSelfAttentionVarSizedElementReduce);
    the query summariser is constructed first, as a caller of the reference constructs it."""
    q = spec["query"]
    if isinstance(q, dict):
        query = build(q, ns)
    elif q == "wsum":
        query = ns.WeightedSumVarSizedElementReduce(spec["D"])
    else:
        query = ns.SimpleVarSizedElementReduce(q)
    if spec["cls"] == "single":
        return ns.SelfAttentionVarSizedElementReduce(spec["D"], spec["hidden"], spec["out"], query)
    return ns.MultiheadSelfAttentionVarSizedElementReduce(spec["D"], spec["hidden"], spec["out"], spec["heads"], query,
                                                          use_value_layer=spec["value"])
