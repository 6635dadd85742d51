"""The fused segment softmax / log-softmax / logsumexp (csrc/segment_softmax.hip) behind `scatter.fused_softmax()`:
both segment-length regimes and every chunk edge against float64, logits spanning 240, the launches taken, and the
facade's any-rank and 16-bit forms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("softmax", "log_softmax", "logsumexp")
LENGTHS = {"short": None,                                    # 300 segments of 0 .. 9 elements
           "boundary": [127, 128, 129, 1, 0, 257, 700],      # both sides of the 128-slot chunk, several chunks
           "wide": [900, 5, 128, 3000, 1, 200]}              # 4234 x 130 values: past the write pass's grid cap


def make(layout, D, seed=0):
    """(src [E, D], shuffled index [E], n) of a named layout; "wide" draws integers of [-120, 120] with some -inf."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 10, (300,), generator=g) if layout == "short" else torch.tensor(LENGTHS[layout])
    if layout == "short":
        lens[:4] = torch.tensor([0, 1, 0, 1])
    n, E = len(lens), int(lens.sum())
    index = torch.repeat_interleave(torch.arange(n), lens)[torch.randperm(E, generator=g)]
    if layout != "wide":
        return torch.randn(E, D, generator=g) * 3, index, n
    src = torch.randint(-120, 121, (E, D), generator=g).float()
    drop = torch.rand(E, D, generator=g) < 0.1
    for s in range(n):                                       # every segment keeps a finite element in every column
        drop[(index == s).nonzero()[0]] = False
    return src.masked_fill(drop, float("-inf")), index, n


@pytest.mark.parametrize("kind,D,layout,eps",
                         [(k, D, lay, eps) for k in KINDS for D in (1, 2, 3, 8, 12, 20, 33, 130)
                          for lay in ("short", "boundary") for eps in (0.0, 1e-12)]
                         + [(k, 3, "short", 0.5) for k in KINDS])
def test_forward_and_gradient_match_float64(kind, D, layout, eps):
    from ptgnn_amd import scatter as S
    src, index, n = make(layout, D)
    xr = src.double().requires_grad_(True)
    sel = [torch.nonzero(index == s).squeeze(1) for s in range(n)]
    parts = []
    for s in range(n):
        xs = xr[sel[s]]
        if xs.shape[0] == 0:
            parts.append(torch.full((D,), float("-inf"), dtype=torch.float64))
        elif eps == 0:
            parts.append({"softmax": torch.softmax, "log_softmax": torch.log_softmax,
                          "logsumexp": torch.logsumexp}[kind](xs, 0))
        else:
            m = xs.max(0).values.detach()
            total = (xs - m).exp().sum(0) + eps
            parts.append({"softmax": (xs - m).exp() / total, "log_softmax": xs - m - total.log(),
                          "logsumexp": total.log() + m}[kind])
    if kind == "logsumexp":
        want = torch.stack(parts)
    else:
        want = torch.zeros(len(index), D, dtype=torch.float64).index_put(
            (torch.cat(sel),), torch.cat([p for p, i in zip(parts, sel) if len(i)]))
    x = src.cuda().requires_grad_(True)
    with S.fused_softmax():
        got = getattr(S, "scatter_" + kind)(x, index.cuda(), dim=0, dim_size=n, eps=eps)
    keep = torch.ones(len(index), dtype=torch.bool)
    if kind == "logsumexp":
        keep = torch.bincount(index, minlength=n) > 0
        assert bool(torch.isneginf(got.detach().cpu()[~keep]).all())
    err = (got.detach().cpu().double()[keep] - want.detach()[keep]).abs().max()
    w = torch.linspace(-1, 1, want.numel()).view_as(want)
    (got[keep.cuda()] * w.cuda()[keep.cuda()]).sum().backward()
    (want[keep] * w.double()[keep]).sum().backward()
    gerr = (x.grad.cpu().double() - xr.grad).abs().max()
    print(f"{kind} D={D} {layout} eps={eps}: forward {float(err):.3g}, gradient {float(gerr):.3g}")
    assert float(err) <= 1e-5 and float(gerr) <= 2e-5


@pytest.mark.parametrize("kind", KINDS)
def test_logits_spanning_240_with_minus_infinities(kind):
    from ptgnn_amd import scatter as S
    src, index, n = make("wide", 130, seed=3)
    xr = src.double().requires_grad_(True)
    fn = {"softmax": torch.softmax, "log_softmax": torch.log_softmax, "logsumexp": torch.logsumexp}[kind]
    sel = [torch.nonzero(index == s).squeeze(1) for s in range(n)]
    want = torch.stack([fn(xr[i], 0) for i in sel]) if kind == "logsumexp" else \
        torch.zeros_like(xr).index_put((torch.cat(sel),), torch.cat([fn(xr[i], 0) for i in sel]))
    x = src.cuda().requires_grad_(True)
    with S.fused_softmax():
        got = getattr(S, "scatter_" + kind)(x, index.cuda(), dim=0, dim_size=n, eps=0.0)
    finite = torch.isfinite(want.detach())
    res = got.detach().cpu().double()
    assert bool(torch.isfinite(res[finite]).all()) and torch.equal(res[~finite], want.detach()[~finite])
    np.testing.assert_allclose(res[finite].numpy(), want.detach()[finite].numpy(), rtol=1e-6, atol=1e-5)
    w = torch.linspace(-1, 1, want.numel()).view_as(want)
    (got * w.cuda()).sum().backward()
    (want * w.double()).sum().backward()
    assert bool(torch.isfinite(x.grad).all())
    at = torch.isneginf(src)
    np.testing.assert_array_equal(x.grad.cpu().double()[at].numpy(), xr.grad[at].numpy())


def test_route_and_determinism():
    from ptgnn_amd import ops, scatter as S
    src, index, n = make("boundary", 8)
    runs = {}
    for on in (True, False, True):
        fwd, both, outs = set(), set(), []
        for kind in KINDS:
            x = src.cuda().requires_grad_(True)
            timer = ops.KernelTimer()
            ops.set_kernel_timer(timer)
            try:
                with S.fused_softmax(on):
                    out = getattr(S, "scatter_" + kind)(x, index.cuda(), dim=0, dim_size=n)
                fwd |= set(timer.summary())
                out.clamp(min=-50).sum().backward()
                both |= set(timer.summary())
            finally:
                ops.set_kernel_timer(None)
            outs += [out.detach(), x.grad]
        if on:
            assert "segment_softmax" in fwd and "gather_reduce" not in fwd, fwd
            assert "segment_softmax_backward" in both, both
            runs.setdefault("fused", []).append(outs)
        else:
            assert not {"segment_softmax", "segment_softmax_backward"} & both and "gather_reduce" in both, both
    first, second = runs["fused"]
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("kind", KINDS)
def test_any_rank_and_16_bit_sources_through_the_facade(kind):
    from ptgnn_amd import scatter as S
    g = torch.Generator().manual_seed(11)
    I, L, H, n = 300, 3, 4, 40
    src = torch.randn(I, L, H, generator=g) * 3
    index = torch.randint(0, n, (I,), generator=g)
    name = "scatter_" + kind
    for d, t in ((0, src), (1, src.permute(1, 0, 2).contiguous())):
        xh = t.double().requires_grad_(True)
        want = getattr(S, name)(xh, index, dim=d, dim_size=n)
        x = t.cuda().requires_grad_(True)
        with S.fused_softmax():
            got = getattr(S, name)(x, index.cuda(), dim=d, dim_size=n)
        assert tuple(got.shape) == tuple(want.shape)
        np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=0, atol=1e-5)
        w = torch.linspace(-1, 1, want.numel()).view_as(want)
        (got.clamp(min=-50) * w.cuda()).sum().backward()
        (want.clamp(min=-50) * w.double()).sum().backward()
        np.testing.assert_allclose(x.grad.cpu().numpy(), xh.grad.numpy(), rtol=0, atol=2e-5)
    for dtype in (torch.bfloat16, torch.float16):
        with S.fused_softmax():
            assert getattr(S, name)(src.cuda().to(dtype), index.cuda(), dim=0, dim_size=n).dtype == dtype
