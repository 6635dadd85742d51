"""Case specs of the GraphNorm fixtures: tests/golden/make_golden_graphnorm.py builds them from the reference's class,
tests/test_graphnorm_cpu.py and tests/test_gpu_graphnorm.py from ptgnn_amd.layers.GraphNorm.

`random_params`: gamma and alpha are drawn from 0.5 + U(0, 1) and bias from N(0, 1), so that the alpha path is exercised
(alpha = 1 removes the mean exactly); without it the layer keeps its initial ones / ones / zeros."""

# nodes per graph: one beyond half a 128-row chunk, a 1-node graph, an empty graph in the middle, a 2-node graph
SIZES = [70, 1, 0, 33, 2]
# GraphNorm reads the number of graphs as index.max() + 1, so a trailing graph can only be empty if a later one is not:
# one more node carries the index PAST the next graph, which leaves graph len(SIZES) empty behind all the others
EXTRA_INDEX = len(SIZES) + 1
NUM_GRAPHS = EXTRA_INDEX + 1
COUNTS = SIZES + [0, 1]

CASES = [
    ("graphnorm_d6", dict(D=6, eps=1e-10, random_params=True, seed=21)),
    ("graphnorm_d64", dict(D=64, eps=1e-10, random_params=True, seed=22)),
    ("graphnorm_d64_default", dict(D=64, eps=1e-10, random_params=False, seed=23)),
    ("graphnorm_d6_eps", dict(D=6, eps=1e-5, random_params=True, seed=24)),
]


def build(spec, ns):
    """The layer of `spec` from the namespace `ns` (a module holding GraphNorm), with its initial parameters."""
    return ns.GraphNorm(spec["D"], eps=spec["eps"])
