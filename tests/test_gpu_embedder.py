"""TokenUnitEmbedder / SubtokenUnitEmbedder on the MI355X: the fused embedding bag (csrc/embedding_bag.hip) against the
reference fixtures, the exact cases (max is a selection, the token embedder a row copy), the kernel against a float64
restatement at every lane-group width, slot count and length class, the backward's long-row and hub thresholds,
determinism, dispatch (launch counters, the composed route beyond the fused range, AMP dtypes) and the modules as the
node embedder of a GraphNeuralNetwork."""
import contextlib
from unittest import mock

import pytest
import torch
from torch import nn

from agg_paths import HUB_THRESHOLD, K_LONG_ROW, TOL, attributed_ok
from embedder_cases import CASES, args_of, build, load, loss_of, ref_pool, state_of
from ptgnn_amd import embeddings, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXTURE_TOL = 2e-5          # the bar of tests/test_gpu_attention_pool.py, relative to max(1, max |want|)
GRAD_TOL = 2e-5             # DESIGN section 6, relative to max |g|
INF = float("inf")
KINDS = ("sum", "mean", "max")


def _refuse(name):
    def raiser(*args, **kwargs):
        raise AssertionError(f"{name} was called on the GPU route")
    return raiser


@contextlib.contextmanager
def no_vendor_calls():
    with mock.patch.object(nn.functional, "embedding", _refuse("F.embedding")), \
            mock.patch.object(nn.functional, "linear", _refuse("F.linear")), \
            mock.patch.object(torch, "index_select", _refuse("torch.index_select")):
        yield


def attributed(got, want32, exact, what):
    """Same -inf positions, finite entries by the attributed rule scaled by max(1, max |float64|)."""
    got, want32, exact = got.detach().cpu(), want32.detach().cpu(), exact.detach().cpu()
    if not (torch.equal(got == -INF, exact == -INF) and torch.equal(want32 == -INF, exact == -INF)):
        return False
    finite = torch.isfinite(exact)
    if not bool(finite.any()):
        return True
    got, want32, exact = got[finite], want32[finite], exact[finite]
    scale = max(1.0, float(exact.abs().max()))
    print(f"    {what}: |got-fp32|={float((got - want32).abs().max()):.3e} "
          f"|got-f64|={float((got.double() - exact).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


def reference(table, ids, lengths, kind, gout, dtype):
    """(pool, d table) of the restatement in `dtype` on the CPU; the loss leaves out the bags without a subtoken."""
    t = table.detach().cpu().to(dtype).requires_grad_(True)
    ids, lengths, gout = ids.cpu(), lengths.cpu(), gout.cpu().to(dtype)
    out = ref_pool(t, ids, lengths, kind)
    keep = lengths > 0
    (out[keep] * gout[keep]).sum().backward()
    return out.detach(), t.grad


def device_pool(table, ids, lengths, kind, gout):
    t = table.detach().clone().requires_grad_(True)
    out = embeddings.embedding_bag(t, ids, lengths, kind)
    keep = lengths > 0
    (out[keep] * gout[keep]).sum().backward()
    return out.detach(), t.grad


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    fx = load(name)
    module = build(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    module = module.to(DEV)
    args, coef = args_of(fx, lambda t: t.to(DEV)), torch.from_numpy(fx["coef"]).to(DEV)
    before = ops.launch_counts(aggregation=True)
    with no_vendor_calls():
        out = module(*args)
        loss_of(out, args, coef).backward()
    since = ops.launches_since(before)
    if spec["kind"] != "token":
        assert since["embedding_bag"] == 1 and since["embedding_bag_backward"] == 1
    want = torch.from_numpy(fx["out"])
    got = out.detach().cpu()
    assert torch.equal(got == -INF, want == -INF)
    finite = torch.isfinite(want)
    err, scale = float((got[finite] - want[finite]).abs().max()), max(1.0, float(want[finite].abs().max()))
    print(f"    out: |got - want| = {err:.3e} (scale {scale:.3e})")
    assert err <= FIXTURE_TOL * scale
    for k, p in module.named_parameters():
        g = torch.from_numpy(fx["grad." + k])
        err = float((p.grad.cpu() - g).abs().max())
        print(f"    {k}: |got - want| = {err:.3e} (max |g| {float(g.abs().max()):.3e})")
        assert err <= GRAD_TOL * float(g.abs().max()), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. exactness that follows from the arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_max_pool_without_the_dense_layer_is_a_selection():
    name, spec = next(c for c in CASES if c[0] == "embedder_max_pool")
    fx = load(name)
    module = build(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    ids, lengths = args_of(fx)
    want = ref_pool(module.embedding_layer.weight.detach(), ids, lengths, "max")           # float32 on the CPU
    with torch.no_grad():
        got = module.to(DEV)(ids.to(DEV), lengths.to(DEV))
    assert bool((want == -INF).any()) and torch.equal(got.cpu(), want)


def test_token_embedder_in_eval_is_a_row_copy():
    name, spec = next(c for c in CASES if c[0] == "embedder_token")
    fx = load(name)
    module = build(spec, embeddings, dropout_rate=0.3)
    module.load_state_dict(state_of(fx), strict=True)
    module = module.to(DEV).eval()
    (ids,) = args_of(fx, lambda t: t.to(DEV))
    with no_vendor_calls(), torch.no_grad():
        got = module(ids)
    assert torch.equal(got, module.embedding_layer.weight.detach()[ids])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the kernel against float64: every lane-group width, slot count, bag count and length class
# ---------------------------------------------------------------------------------------------------------------------
def sweep_inputs(B, S, V, D, seed):
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(V, D, generator=gen)
    ids = torch.randint(0, V - 3, (B, S), generator=gen)         # the last three vocabulary rows are never referenced
    classes = [S, 0, 1, S + 2] if B != 3 else [0, 1, S + 2]      # B = 1: S;  B = 3: 0, 1, S + 2;  B = 257: all, cycled
    lengths = torch.tensor([classes[b % len(classes)] for b in range(B)], dtype=torch.int64)
    if S >= 2:
        ids[0, 1] = ids[0, 0]                                    # a tie of the max on one table row
        ids[B - 1, S - 1] = ids[B - 1, 0]
    gout = torch.randn(B, D, generator=gen)
    return table, ids, lengths, gout


@pytest.mark.parametrize("D", (4, 8, 64, 128, 132, 1024))
@pytest.mark.parametrize("S", (1, 5, 32))
def test_kernel_sweep_against_float64(D, S):
    assert ops.embedding_bag_supported(D, S)
    V = 41
    seen = set()
    for B in (1, 3, 257):
        table, ids, lengths, gout = sweep_inputs(B, S, V, D, seed=1000 * D + 10 * S + B)
        seen |= set(lengths.tolist())
        dev = [t.to(DEV) for t in (table, ids, lengths)]
        for kind in KINDS:
            o32, g32 = reference(table, ids, lengths, kind, gout, torch.float32)
            o64, g64 = reference(table, ids, lengths, kind, gout, torch.float64)
            before = ops.launch_counts(aggregation=True)
            out, grad = device_pool(*dev, kind, gout.to(DEV))
            since = ops.launches_since(before)
            assert since["embedding_bag"] == 1 and since["embedding_bag_backward"] == 1
            assert attributed(out, o32, o64, f"B={B} {kind} out"), (B, kind)
            assert attributed(grad, g32, g64, f"B={B} {kind} d table"), (B, kind)
            assert not grad[-3:].any()                           # rows nobody references: exactly 0
            if kind == "max":
                assert torch.equal(out.cpu(), o32)               # a selection
    assert seen >= {0, 1, S, S + 2}


# ---------------------------------------------------------------------------------------------------------------------
# 4. the backward's row paths: tokens that occur 255 .. 2049 times, and a padding row beyond the hub threshold
# ---------------------------------------------------------------------------------------------------------------------
COUNTS = (K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1, HUB_THRESHOLD - 1, HUB_THRESHOLD, HUB_THRESHOLD + 1)


def threshold_bag(D=64, S=5, V=64, seed=7):
    """Live bags whose slots hold token k exactly COUNTS[k] times (k < 6) between background tokens, shuffled; then
    short bags over background tokens only, and 520 empty bags, whose 2600 dead slots make the padding row a hub."""
    gen = torch.Generator().manual_seed(seed)
    special = torch.cat([torch.full((c,), k, dtype=torch.int64) for k, c in enumerate(COUNTS)])
    full = 1600
    background = torch.randint(len(COUNTS), V - 3, (full * S - special.shape[0],), generator=gen)
    flat = torch.cat((special, background))
    flat = flat[torch.randperm(flat.shape[0], generator=gen)]
    short = torch.randint(len(COUNTS), V - 3, (20, S), generator=gen)
    ids = torch.cat((flat.reshape(full, S), short, torch.randint(0, V, (520, S), generator=gen)))
    lengths = torch.cat((torch.full((full,), S), torch.arange(20) % S, torch.zeros(520, dtype=torch.int64)))
    B = ids.shape[0]
    return torch.randn(V, D, generator=gen), ids, lengths.to(torch.int64), torch.randn(B, D, generator=gen)


@pytest.fixture(scope="module")
def threshold_case():
    table, ids, lengths, gout = threshold_bag()
    live = torch.arange(ids.shape[1]).unsqueeze(0) < lengths.unsqueeze(1)
    counts = torch.bincount(ids[live], minlength=table.shape[0])
    assert counts[:len(COUNTS)].tolist() == list(COUNTS) and int((~live).sum()) > HUB_THRESHOLD
    refs = {(kind, dt): reference(table, ids, lengths, kind, gout, dt)
            for kind in ("sum", "mean") for dt in (torch.float32, torch.float64)}
    return table, ids, lengths, gout, refs


@pytest.mark.parametrize("kind", ("sum", "mean"))
def test_backward_long_rows_and_hub_rows_against_float64(threshold_case, kind):
    table, ids, lengths, gout, refs = threshold_case
    (o32, g32), (o64, g64) = refs[(kind, torch.float32)], refs[(kind, torch.float64)]
    out, grad = device_pool(table.to(DEV), ids.to(DEV), lengths.to(DEV), kind, gout.to(DEV))
    assert attributed(out, o32, o64, f"{kind} out")
    assert attributed(grad, g32, g64, f"{kind} d table")
    assert not grad[-3:].any()


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_identical_bits(threshold_case, kind):
    table, ids, lengths, gout, _ = threshold_case
    dev = [t.to(DEV) for t in (table, ids, lengths)]
    first = device_pool(*dev, kind, gout.to(DEV))
    second = device_pool(*dev, kind, gout.to(DEV))
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. dispatch
# ---------------------------------------------------------------------------------------------------------------------
def test_one_bag_launch_per_forward_and_the_backward_family_in_training():
    ids = torch.randint(0, 30, (50, 5), device=DEV)
    lengths = torch.randint(1, 6, (50,), device=DEV)
    for kind in KINDS:
        module = embeddings.SubtokenUnitEmbedder(30, 64, 0.0, kind, use_dense_output=False).to(DEV)
        before = ops.launch_counts(aggregation=True)
        with torch.no_grad():
            module.eval()(ids, lengths)
        assert ops.launches_since(before) == {"embedding_bag": 1}
        before = ops.launch_counts(aggregation=True)
        module.train()(ids, lengths).sum().backward()
        want = {"embedding_bag": 1, "embedding_bag_backward": 1}
        if kind != "max":
            want["k_gather_reduce"] = 1          # the row walk of the sum; max takes the arg-routed reduce
        assert ops.launches_since(before) == want


@pytest.mark.parametrize("D,S", ((127, 5), (64, 33)))
def test_composed_route_beyond_the_fused_range_matches_float64(D, S):
    assert not ops.embedding_bag_supported(D, S)
    B, V = 37, 41
    table, ids, lengths, gout = sweep_inputs(B, S, V, D, seed=D + S)
    for kind in KINDS:
        module = embeddings.SubtokenUnitEmbedder(V, D, 0.0, kind, use_dense_output=False).to(DEV)
        with torch.no_grad():
            module.embedding_layer.weight.copy_(table)
        o32, g32 = reference(table, ids, lengths, kind, gout, torch.float32)
        o64, g64 = reference(table, ids, lengths, kind, gout, torch.float64)
        before = ops.launch_counts(aggregation=True)
        with mock.patch.object(nn.functional, "embedding", _refuse("F.embedding")):
            out = module(ids.to(DEV), lengths.to(DEV))
            keep = (lengths > 0).to(DEV)
            (out[keep] * gout.to(DEV)[keep]).sum().backward()
        assert "embedding_bag" not in ops.launches_since(before)
        assert attributed(out, o32, o64, f"{kind} out")
        assert attributed(module.embedding_layer.weight.grad, g32, g64, f"{kind} d table")


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
def test_half_tables_round_trip_their_dtype(dtype):
    ids = torch.randint(0, 30, (20, 5), device=DEV)
    lengths = torch.randint(1, 6, (20,), device=DEV)
    for kind, dense in (("mean", True), ("max", False)):
        torch.manual_seed(5)
        half = embeddings.SubtokenUnitEmbedder(30, 64, 0.0, kind, use_dense_output=dense).to(DEV).to(dtype)
        full = embeddings.SubtokenUnitEmbedder(30, 64, 0.0, kind, use_dense_output=dense).to(DEV)
        full.load_state_dict({k: v.float() for k, v in half.state_dict().items()})
        out = half(ids, lengths)
        out.float().sum().backward()
        assert out.dtype == dtype and all(p.grad.dtype == dtype for p in half.parameters())
        with torch.no_grad():
            assert torch.equal(out.detach(), full(ids, lengths).to(dtype))
    token = embeddings.TokenUnitEmbedder(30, 64, 0.0).to(DEV).to(dtype)
    out = token(ids[:, 0])
    assert out.dtype == dtype and torch.equal(out.detach(), token.embedding_layer.weight.detach()[ids[:, 0]])


@pytest.mark.parametrize("kind", ("subtoken", "token"))
def test_node_embedder_of_a_two_layer_ggnn(kind):
    from ptgnn_amd import layers as L, workloads
    from ptgnn_amd.gnn import GraphNeuralNetwork
    mb = workloads.batched_graphs(3, 60, 3, 2.2, seed=3)
    N, H, T, V = mb["num_nodes"], 64, 7, 50
    torch.manual_seed(0)
    if kind == "subtoken":
        embedder = embeddings.SubtokenUnitEmbedder(V, H, 0.0, "mean")
        node_data = {"token_idxs": torch.randint(0, V - 3, (N, 5), device=DEV),
                     "lengths": torch.randint(1, 6, (N,), device=DEV)}
    else:
        embedder = embeddings.TokenUnitEmbedder(V, H, 0.0)
        node_data = {"token_idxs": torch.randint(0, V - 3, (N,), device=DEV)}
    net = GraphNeuralNetwork([L.GatedMessagePassingLayer(H, H, T, "max"), L.GatedMessagePassingLayer(H, H, T, "sum")],
                             embedder, True, True).to(DEV)
    before = ops.launch_counts(aggregation=True)
    with mock.patch.object(nn.functional, "embedding", _refuse("F.embedding")):
        out = net(node_data=node_data, adjacency_lists=[(s.to(DEV), d.to(DEV)) for s, d in mb["adjacency_lists"]],
                  edge_feature_data=[], node_to_graph_idx=mb["node_to_graph_idx"].to(DEV),
                  reference_node_ids={k: v.to(DEV) for k, v in mb["reference_node_ids"].items()},
                  reference_node_graph_idx={k: v.to(DEV) for k, v in mb["reference_node_graph_idx"].items()},
                  num_graphs=mb["num_graphs"])
        states = out.output_node_representations
        states.square().sum().backward()
    since = ops.launches_since(before)
    if kind == "subtoken":
        assert since["embedding_bag"] == 1 and since["embedding_bag_backward"] == 1
    grad = embedder.embedding_layer.weight.grad
    assert tuple(states.shape) == (N, H) and bool(torch.isfinite(states).all())
    assert bool(torch.isfinite(grad).all()) and bool(grad[:V - 3].any()) and not grad[V - 3:].any()
