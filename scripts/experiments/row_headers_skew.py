"""Header-first aggregation walk against the plain walk on graphs whose rows mostly exceed one group of 8 in-edges.

    python scripts/experiments/row_headers_skew.py

The header walk fetches the col entries of slots 8.. at the top of each further group; this prints the per-launch time
of ops.gather_reduce (HIP events, 30 launches each, the two walks alternating) with and without row headers for
in-degree distributions capped at the long-row threshold (256), plus the bit comparison of the two outputs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from ptgnn_amd import ops  # noqa: E402


def graph(n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "deg9-16":
        deg = torch.randint(9, 17, (n,), generator=g)
    elif kind == "deg17-64":
        deg = torch.randint(17, 65, (n,), generator=g)
    else:   # heavy tail: 1 + floor of a Pareto draw, capped at 256 (mean ~ 12, 40 % of the rows above 8)
        u = torch.rand(n, generator=g).clamp_min(1e-6)
        deg = (4.0 * u.pow(-1.0 / 1.3)).floor().clamp(1, 256).long()
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(dst.numel()),), generator=g)
    return [(src.cuda(), dst.cuda())], deg


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1000.0 / reps


def main():
    n, m = 100_000, 128
    for kind in ("deg9-16", "deg17-64", "pareto<=256"):
        adj, deg = graph(n, kind, 7)
        plan = ops.build_plan(adj, n)
        y = torch.randn(n, m, device="cuda")
        out = {}
        for reduce in ("max", "sum"):
            def run(header):
                ops.ROW_HEADERS = header
                return ops.gather_reduce(y, plan, m, reduce)
            for header in (True, False):
                out[header] = run(header)
            same = torch.equal(out[True].view(torch.int32), out[False].view(torch.int32))
            t = {True: [], False: []}
            for _ in range(3):
                for header in (False, True):
                    t[header].append(timed(lambda: run(header), 30))
            print(f"{kind:12s} {reduce:4s} E={int(deg.sum())} mean_deg={float(deg.float().mean()):.1f} "
                  f"plain_us={min(t[False]):.1f} header_us={min(t[True]):.1f} same_bits={same}", flush=True)


if __name__ == "__main__":
    main()
