"""Child process of tests/test_gpu_aggregation_paths.py: the hub launches that only large plans take by default.

PTGNN_AMD_SIDE_MIN_EDGES and PTGNN_AMD_HUB_STREAM are read once per process, so this script runs with them set:
  * PTGNN_AMD_SIDE_MIN_EDGES=0: k_hub_chunks and k_long_rows on the library's side streams, for every plan;
  * PTGNN_AMD_SIDE_MIN_EDGES=0 PTGNN_AMD_HUB_STREAM=0: the dedicated k_hub_chunks launch on the caller's stream.
On the degree-spectrum graphs of tests/agg_paths.py it checks gather_reduce (plain, destination term at T = 1, max
with arg) and gather_combine against the oracle with the bars of the test module (hub-row sums: float64 only; the
fused and dedicated hub launches promise no bit equality with each other), then saves its outputs to argv[1] so the
parent can compare the rows of degree <= 2048 with its own default path.  Prints "side-check ok" on success."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import agg_paths as AP  # noqa: E402

M = 64
K, B, DH = 2, 2, 16


def inputs(sp, name):
    """Deterministic inputs of case `name` on the CPU: (y, ydst or None, coef or None)."""
    reduce = "max" if name.endswith(("max", "arg")) else "sum"
    T = sp.num_types
    if name.startswith("edge") or name.startswith("egc"):
        rows = sp.num_edges
    else:
        rows = sp.num_nodes
    cols = M if rows == sp.num_edges else T * M
    y = AP.tie_values(rows, cols, seed=7) if reduce == "max" else \
        torch.randn(rows, cols, generator=torch.Generator().manual_seed(7))
    yd = torch.randn(sp.num_nodes, T * M, generator=torch.Generator().manual_seed(8)) if "dst" in name else None
    coef = torch.randn(sp.num_nodes, K * B, generator=torch.Generator().manual_seed(9)) if name.startswith("egc") \
        else None
    return y, yd, coef


def _edge(plan, inp, reduce, arg):
    from ptgnn_amd import ops
    res = ops.gather_reduce(inp[0].cuda(), plan, M, reduce, type_bits=0, col=plan.perm, return_arg=arg)
    return list(res) if arg else [res]


def _dst(plan, inp):
    from ptgnn_amd import ops
    return [ops.gather_reduce(inp[0].cuda(), plan, M, "sum", ydst=inp[1].cuda())]


def _egc(plan, inp, reduce):
    from ptgnn_amd import ops
    out, agg, arg = ops.gather_combine(inp[0].cuda(), plan, K, B, DH, reduce, inp[2].cuda(), type_bits=0,
                                       col=plan.perm, return_agg=True, return_arg=reduce == "max")
    return [out, agg, arg]


# name -> (edge types, fn(plan, inputs) -> list of output tensors)
CASES = {
    "edge_sum": (1, lambda p, i: _edge(p, i, "sum", False)),
    "edge_max": (1, lambda p, i: _edge(p, i, "max", False)),
    "edge_arg": (1, lambda p, i: _edge(p, i, "max", True)),
    "table_dst_sum": (1, _dst),
    "egc_sum": (1, lambda p, i: _egc(p, i, "sum")),
    "egc_max": (1, lambda p, i: _egc(p, i, "max")),
}


def _check(sp, name, res, inp):
    from oracle import scatter_ref
    src, dst, typ = sp.src_dst_type()
    N, E = sp.num_nodes, sp.num_edges
    y, yd, coef = inp
    msgs = y if y.shape[0] == E else y.view(N, sp.num_types, M)[src, typ]
    if yd is not None:
        msgs = msgs + yd.view(N, sp.num_types, M)[dst, typ]
    agg = res[1] if name.startswith("egc") else res[0]
    got = agg.cpu()
    small = sp.deg <= AP.HUB_THRESHOLD
    if name.endswith(("max", "arg")):
        want, want_arg = AP.first_winner(msgs, dst, N, "max")
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, "max value bits")
        arg = res[2] if name.startswith("egc") else (res[1] if len(res) > 1 else None)
        if arg is not None:
            return arg, want_arg, want
    else:
        want32 = scatter_ref.scatter(msgs, dst, dim=0, dim_size=N, reduce="sum")
        assert torch.equal(got[small].view(torch.int32), want32[small].view(torch.int32)), (name, "serial bits")
        want64 = scatter_ref.scatter(msgs.double(), dst, dim=0, dim_size=N, reduce="sum")
        mass = scatter_ref.scatter(msgs.double().abs(), dst, dim=0, dim_size=N, reduce="sum")
        err = float(((got.double() - want64).abs() / (1.0 + mass))[~small].max())
        assert err <= 5e-6, (name, "hub rows vs float64", err)
    return None


def main(dump):
    from ptgnn_amd import ops
    assert torch.cuda.is_available()
    sp = AP.spectrum_graph(num_types=1)
    plan = ops.build_plan([(s.cuda(), d.cuda()) for s, d in sp.adj], sp.num_nodes)
    assert plan.may_have_hubs() and int(plan.hub_count.reshape(-1)[0]) > 0
    assert bool(((sp.deg > AP.K_LONG_ROW) & (sp.deg <= AP.HUB_THRESHOLD)).any())   # rows for k_long_rows
    perm = plan.perm[: sp.num_edges].cpu().long()
    saved = {}
    for name, (T, fn) in CASES.items():
        assert T == sp.num_types
        inp = inputs(sp, name)
        res = fn(plan, inp)
        again = fn(plan, inp)
        for a, b in zip(res, again):
            if a is None:
                continue
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "two runs differ")
        torch.cuda.synchronize()
        assert int(plan.hub_tickets(M).abs().sum()) == 0, (name, "tickets left nonzero")
        arg_check = _check(sp, name, res, inp)
        if arg_check is not None:
            arg, want_arg, _ = arg_check
            a = arg.cpu().long()
            got_edge = torch.where(a >= 0, perm[a.clamp(min=0)], torch.full_like(a, sp.num_edges))
            assert torch.equal(got_edge, want_arg), (name, "arg")
        if name.startswith("egc"):
            c64 = torch.einsum("nkb,nkbd->nkd", inp[2].double().view(-1, K, B),
                               res[1].cpu().double().view(-1, K, B, DH)).reshape(-1, K * DH)
            mass = torch.einsum("nkb,nkbd->nkd", inp[2].double().abs().view(-1, K, B),
                                res[1].cpu().double().abs().view(-1, K, B, DH)).reshape(-1, K * DH)
            assert float(((res[0].cpu().double() - c64).abs() / (1.0 + mass)).max()) <= 1e-6, (name, "combine")
        saved[name] = [r.cpu() if r is not None else None for r in res]
        print(f"{name}: ok", flush=True)
    torch.save(saved, dump)
    env = {k: os.environ.get(k) for k in ("PTGNN_AMD_SIDE_MIN_EDGES", "PTGNN_AMD_HUB_STREAM")}
    print(f"side-check ok {env} cases={len(saved)}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
