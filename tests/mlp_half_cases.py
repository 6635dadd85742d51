"""Test support for the opt-in 16-bit matrix inputs of the MLP-MP layer (`ptgnn_amd.matrix_inputs(dtype, mlp=True)`,
csrc/edge_gemm16.hip with a target-state half), on top of tests/half_cases.py: float64 restatements of the message
Linear over [x[src] | x[dst]] and of the layer (mlpmessagepassing.py:81-117) with ONLY the message operands rounded, and
the case builders the GPU and the CPU tests share.  Reference, bar and precondition: tests/half_cases.py.  Never imported
by the product package.

LayerNorm follows the aggregation in this layer, and it is continuous in the messages (unlike the GRU of the GGNN layer
it rounds nothing it computed), so the restatement needs no captured intermediate: every case here was chosen, on the
CPU, such that the exact-fp32 CPU route is inside the bar of float64 -- the LayerNorm of these inputs does not amplify an
fp32 rounding beyond it -- and such that rounding moves the result by >= MARGIN bars.
"""
import torch

import half_cases as C
from agg_paths import pna_ref

UNIT_ROWS = (0, 1, 31, 32, 33, 97, 0, 64)        # empty types, a single row, both sides of a 32-row unit
N_NODES = 120


def check(got, rounded, exact, what):
    """The precondition on the inputs, then the two assertions on the result (as tests/test_gpu_edge_inputs.py)."""
    bar = C.bar(rounded)
    gap = C.err(exact, rounded)
    e, e_exact = C.err(got, rounded), C.err(got, exact)
    print(f"  {what}: bar {bar:.3e} gap {gap:.3e} |got - rounded| {e:.3e} |got - exact| {e_exact:.3e}")
    assert gap >= C.MARGIN * bar, f"{what}: inputs do not tell the references apart ({gap:.3e} < 20 x {bar:.3e})"
    assert e <= bar, f"{what}: {e:.3e} > {bar:.3e}"
    assert e_exact >= gap - bar, what


def adjacency(n, counts, seed, dst_pool=None):
    """Per type counts[t] edges with src and dst drawn independently, src != dst on every edge.  `dst_pool`: the targets
    are the first dst_pool nodes only (the sources the others), so that a node with any message has several."""
    g = torch.Generator().manual_seed(seed)
    adj = []
    for c in counts:
        if dst_pool is None:
            s = torch.randint(0, n, (c,), generator=g)
            d = (s + torch.randint(1, n, (c,), generator=g)) % n
        else:
            s, d = torch.randint(dst_pool, n, (c,), generator=g), torch.randint(0, dst_pool, (c,), generator=g)
        adj.append((s, d))
    return adj


def messages64(x, adj, ws, use_dst=True, dt=None, act=None):
    """act([rnd(x)[src] | rnd(x)[dst]] rnd(W_t)^T) per type in float64, type-major rows; `dt` None: nothing rounded."""
    xr = C.rnd64(x, dt)
    out = []
    for (s, d), w in zip(adj, ws):
        s, d = s.cpu(), d.cpu()
        inp = torch.cat([xr[s], xr[d]], dim=1) if use_dst else xr[s]
        out.append(C.act64(inp @ C.rnd64(w, dt).t(), act))
    return torch.cat(out) if out else torch.zeros(0, ws[0].shape[0], dtype=torch.float64)


def mlp64(x, adj, weights, dt=None, pna_delta=None):
    """mlpmessagepassing.py:81-117 in float64 over `layer.export_weights()` (single-Linear edge transforms): messages
    with the operands rounded to `dt`, the aggregation (`weights["agg"]`: "sum" / "max", or PNA with `pna_delta`), erf
    GELU, LayerNorm (eps 1e-5), Linear + Tanh -- everything after the messages unrounded."""
    F = torch.nn.functional
    msgs = messages64(x, adj, [w[0] for w in weights["edge_mlp"]], weights["use_target"], dt)
    targets = torch.cat([d.cpu() for _, d in adj])
    n = x.shape[0]
    agg = pna_ref(msgs, targets, n, pna_delta) if pna_delta is not None else C.aggregate64(msgs, targets, n,
                                                                                          weights["agg"])
    if weights["gelu"]:
        agg = F.gelu(agg)
    if weights["ln_w"] is not None:
        agg = F.layer_norm(agg, (agg.shape[1],), weights["ln_w"].double(), weights["ln_b"].double(), 1e-5)
    if weights["dense_w"] is not None:
        agg = agg @ weights["dense_w"].double().t() + weights["dense_b"].double()
        if weights["tanh"]:
            agg = torch.tanh(agg)
    return agg


# form -> (edge types, per-type edge counts): `_prefer_edge_path` takes the edge form when 1.25 E < N T
FORMS = {"edge": UNIT_ROWS, "table": (150, 210)}


def layer_case(form, hidden, reduce, use_dst, seed, pna=False):
    """(layer in eval mode on the CPU, states, adjacency): N(0, 1) states, the layer's own Xavier initialisation.
    `pna`: PnaMessageAggregation(delta=1.5) over PNA_TARGETS target nodes -- its "std" is sqrt(sum relu(m^2 - mean^2)),
    which for a node with ONE message is the square root of a cancellation (m^2 - m^2 / (1 + 1e-5)^2) and turns one
    fp32 rounding of m^2 into an error of the size of the bar, in the exact-fp32 routes too; with 258 - 360 edges onto 24
    targets every target has several messages."""
    from ptgnn_amd import layers as L
    counts = FORMS[form]
    torch.manual_seed(seed)
    agg = L.PnaMessageAggregation(delta=1.5) if pna else reduce
    layer = L.MlpMessagePassingLayer(hidden, hidden, hidden, len(counts), agg,
                                     use_target_state_as_message_input=use_dst).eval()
    x = torch.randn(N_NODES, hidden, generator=torch.Generator().manual_seed(seed + 1))
    adj = adjacency(N_NODES, counts, seed + 2, dst_pool=PNA_TARGETS if pna else None)
    if pna:
        assert int(torch.bincount(torch.cat([d for _, d in adj]), minlength=PNA_TARGETS)[:PNA_TARGETS].min()) >= 2
    return layer, x, adj


def run_layer(layer, x, adj, feats=None):
    from ptgnn_amd import ops
    if x.is_cuda:
        ops.clear_plan_cache()
    if feats is None:
        feats = [torch.empty(int(s.shape[0]), 0, device=x.device) for s, _ in adj]
    return layer(x, adj, None, {}, {}, feats)


# The layer cases of the GPU tests: (form, hidden, reduce, use_dst) -> seed.  tests/test_mlp_inputs_cpu.py holds every one
# of them to the two preconditions above on the CPU (fp32 route inside the bar; rounding >= MARGIN bars away).
LAYER_SEEDS = {(form, hidden, reduce, use_dst): 5000 + 100 * i
               for i, (form, hidden, reduce, use_dst) in enumerate(
                   (f, h, r, u) for f in ("edge", "table") for h in (64, 128) for r in ("sum", "max")
                   for u in (True, False))}
PNA_TARGETS = 24
PNA_SEEDS = {"edge": 6100, "table": 6200}
