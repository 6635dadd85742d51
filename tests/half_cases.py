"""Test support for the opt-in 16-bit matrix inputs (ptgnn_amd/precision.py, csrc/half_gemm.hip): float64 restatements
of the Linear, the GRU cell and the GGNN layer on ROUNDED operands, the project's bar, and case builders.  Never imported
by the product package.

Reference and bar.  A product of two bf16 / fp16 values is exact in fp32, so on the operands the kernels round only the
fp32 accumulation and the shared gate math separate a result from float64 on those same rounded operands: the bar is the
project's own `TOL * max(1, |want|inf)` (tests/dense_paths.py).  The float64 reference on the UNROUNDED operands is far
away on that scale (bf16: 6.6e-3 - 8.6e-3, fp16: 0.9e-3 - 1.0e-3 at K = 64 / 128 with N(0, 1) states and Xavier weights,
against a bar of 3e-5 - 4e-5), which every numeric test first checks as a precondition on its inputs (`gap >= 20 bar`)
and then uses: a result within the bar of the rounded reference is at least `gap - bar` from the exact one, so a route
that quietly ran the fp32 kernels fails.

Rounding is not continuous.  Where a route rounds a value it COMPUTED (the GRU rounds the fp32 aggregate of the
messages), a float64 restatement that rounds its own float64 aggregate can land on the neighbouring 16-bit value
whenever the two aggregates -- one fp32 rounding apart, ~6e-8 relative -- straddle a rounding boundary (spacing 2^-8
relative for bf16, 2^-11 for fp16): expected once in a few tens of thousands of elements, and then worth 1e-4 in an
output, several bars.  So `ggnn64` takes the fp32 aggregate the route itself rounded (`agg=`, captured by the test at
the aggregation's return) as the GRU operand, and the test checks that aggregate against float64 separately: each stage
is compared with float64 on exactly the operands that stage rounds.
"""
import contextlib

import torch

from dense_paths import TOL

HALF = (torch.bfloat16, torch.float16)
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}
MARGIN = 20          # precondition: the exact and the rounded float64 references are >= MARGIN bars apart


def bar(want: torch.Tensor) -> float:
    return TOL * max(1.0, float(want.abs().max())) if want.numel() else TOL


def err(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.detach().double().cpu() - want.double().cpu()).abs().max()) if want.numel() else 0.0


def rnd64(t: torch.Tensor, dt) -> torch.Tensor:
    """The float64 value of `t` rounded to `dt` as tensor.to(dtype) rounds it; None / float32: `t` itself."""
    t = t.detach().cpu()
    return t.double() if dt in (None, torch.float32) else t.to(dt).double()


def act64(y, act):
    return torch.tanh(y) if act == "tanh" else (torch.relu(y) if act == "relu" else y)


def linear64(x, w, b=None, act=None, dt=None):
    y = rnd64(x, dt) @ rnd64(w, dt).t()
    if b is not None:
        y = y + b.detach().cpu().double()
    return act64(y, act)


def gru64(a, h, w_ih, w_hh, b_ih, b_hh, dt=None):
    """torch.nn.GRUCell in float64 with the gate GEMMs' operands rounded to `dt` and the UNROUNDED h in the blend."""
    gi = rnd64(a, dt) @ rnd64(w_ih, dt).t() + b_ih.detach().cpu().double()
    gh = rnd64(h, dt) @ rnd64(w_hh, dt).t() + b_hh.detach().cpu().double()
    hd = h.shape[1]
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
    return (1.0 - z) * n + z * h.detach().cpu().double()


def aggregate64(msgs, targets, n, reduce):
    out = torch.zeros(n, msgs.shape[1], dtype=torch.float64)
    if reduce == "sum":
        return out.index_add_(0, targets, msgs)
    assert reduce == "max"
    return out.scatter_reduce_(0, targets.unsqueeze(1).expand_as(msgs), msgs, "amax", include_self=False)


def ggnn64(x, adj, weights, linear_dt=None, gru_dt=None, agg=None):
    """gatedmessagepassing.py:46-69 in float64 over `layer.export_weights()`: per type rnd(x)[src] rnd(W_t)^T, the
    aggregation `weights["agg"]` onto the targets (empty rows 0), the GRU cell of `gru64`.  `agg`: the fp32 aggregate a
    route produced, used as the GRU's operand in place of this function's own (see the module docstring).
    Returns (new states, the float64 aggregate of this function)."""
    x = x.detach().cpu()
    adj = [(s.cpu(), d.cpu()) for s, d in adj]
    msgs = torch.cat([linear64(x, w, dt=linear_dt)[s] for (s, _), w in zip(adj, weights["edge_w"])])
    agg64 = aggregate64(msgs, torch.cat([d for _, d in adj]), x.shape[0], weights["agg"])
    out = gru64(agg64 if agg is None else agg, x, weights["w_ih"], weights["w_hh"], weights["b_ih"], weights["b_hh"],
                dt=gru_dt)
    return out, agg64


def random_adjacency(n, counts, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, n, (c,), generator=g), torch.randint(0, n, (c,), generator=g)) for c in counts]


def xavier(n_out, k, g):
    bound = (6.0 / (n_out + k)) ** 0.5
    return (torch.rand(n_out, k, generator=g) * 2 - 1) * bound


def gru_case(rows, m, hd, seed):
    """N(0, 1) aggregate and state, Xavier weights, small biases: (a, h, w_ih, w_hh, b_ih, b_hh) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, m, generator=g), torch.randn(rows, hd, generator=g), xavier(3 * hd, m, g),
            xavier(3 * hd, hd, g), torch.randn(3 * hd, generator=g) * 0.1, torch.randn(3 * hd, generator=g) * 0.1)


def integer_case(rows, k, n_out, seed):
    """x in [-8, 8], W in [-2, 2], b in [-4, 4], all integers: every product and partial sum is an integer below 2^24
    (|sum| <= 96 * 16 + 4), exact in bf16, fp16 and fp32 -- the result does not depend on any rounding or order."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (rows, k), generator=g).float(), torch.randint(-2, 3, (n_out, k), generator=g).float(),
            torch.randint(-4, 5, (n_out,), generator=g).float())


@contextlib.contextmanager
def captured(monkeypatch, module, name):
    """Record what `module.name` returns while the block runs (the fp32 aggregate a route rounds next)."""
    seen = []
    real = getattr(module, name)

    def wrapper(*args, **kwargs):
        out = real(*args, **kwargs)
        seen.append(out)
        return out
    with monkeypatch.context() as mp:
        mp.setattr(module, name, wrapper)
        yield seen
