"""Cases and float64 restatements for the 16-bit matrix-core inputs of the block attention (ptgnn_amd/precision.py,
`attention=True`; csrc/block_attention16.hip).  Support for tests/test_attention_inputs.py and
tests/test_gpu_attention_inputs.py; never imported by the package.

Two restatements of selfattmessagepassing.py:104-117 per window and head, both float64:

    exact     k, q, v as they are
    rounded   k, q, v rounded to the 16-bit type (round to nearest even, `tensor.to(dtype)`), everything after that in
              float64 with the probabilities P UNROUNDED

The kernel differs from `rounded` by three things only: the rounding of every unnormalised probability (at most u
relative: u = 2^-8 for bf16, 2^-11 for fp16, round to nearest), fp16 gradual underflow (at most 2^-25 absolute per
probability; bf16 has fp32's exponent range) and fp32 arithmetic.  The sum l is taken over the unrounded
probabilities, so for element (k, d)

    |got - rounded| <= u (P |rnd(V)|)[k, d] + n_window tiny max|V| + TOL max(1, |rounded|max)

with TOL the forward bar of tests/dense_paths.py.  The bound is derived, never fitted to what the kernel gives.  The CPU
route rounds P after the normalisation (one rounding more: P / l is rounded, not P): the same bound with 2 u."""
import math

import torch

from dense_paths import TOL

UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}

WIDTHS = [(32, 32), (17, 6), (16, 48), (64, 128), (128, 64), (8, 8), (1, 1)]     # (dk, dv)
HEADS = [1, 3]
# (graph sizes, max_num_nodes): windows of 1, 31, 32, 33 rows, an empty graph between two others, 70 = 33 + 33 + 4;
# and one window of 97 rows (four tiles, the last one with a single row)
BATCHES = {"max33": ([1, 31, 0, 32, 33, 70], 33), "w97": ([97], 250)}


def bounds(counts, max_num_nodes):
    """[(first row, end row)] of the windows: a graph is cut every max_num_nodes rows."""
    out, first = [], 0
    for count in counts:
        out += [(first + lo, first + min(lo + max_num_nodes, count)) for lo in range(0, count, max_num_nodes)]
        first += count
    return out


def make_kqv(counts, heads, dk, dv, seed):
    """fp32 kqv [N, heads (2 dk + dv)]: values N(0, 1), keys and queries N(0, 1) * 3 (rounding them moves the scores)."""
    g = torch.Generator().manual_seed(seed)
    n = sum(counts)
    kqv = torch.randn(n, heads, 2 * dk + dv, generator=g)
    kqv[..., :2 * dk] *= 3.0
    return kqv.reshape(n, heads * (2 * dk + dv)).contiguous()


def rnd(t, dt):
    return t.to(dt).double()


def attention64(kqv, windows, heads, dk, dv, dt=None, round_probs=False):
    """float64 attention of fp32 `kqv` over `windows` = [(lo, hi)]: dt None = `exact`, else `rounded` to dt (with
    `round_probs` also the NORMALISED probabilities: what the CPU route does).
    -> out [N, heads dv], lse [N, heads], weight [N, heads dv] = (P |rnd(V)|), length [N] = rows of the row's window."""
    n = kqv.shape[0]
    x = (kqv if dt is None else kqv.to(dt)).double().reshape(n, heads, 2 * dk + dv)
    out = torch.zeros(n, heads, dv, dtype=torch.float64)
    weight = torch.zeros(n, heads, dv, dtype=torch.float64)
    lse = torch.zeros(n, heads, dtype=torch.float64)
    length = torch.zeros(n, dtype=torch.float64)
    for lo, hi in windows:
        k, q, v = (x[lo:hi, :, :dk], x[lo:hi, :, dk:2 * dk], x[lo:hi, :, 2 * dk:])
        s = torch.einsum("khd,vhd->khv", k, q) / math.sqrt(dk)
        lse[lo:hi] = torch.logsumexp(s, dim=-1)
        p = torch.softmax(s, dim=-1)
        if round_probs:
            p = rnd(p.float(), dt)
        out[lo:hi] = torch.einsum("khv,vhd->khd", p, v)
        weight[lo:hi] = torch.einsum("khv,vhd->khd", p, v.abs())
        length[lo:hi] = hi - lo
    return out.reshape(n, heads * dv), lse, weight.reshape(n, heads * dv), length


def out_bound(rounded, weight, length, vmax, dt, roundings=1):
    """The elementwise bound on |got - rounded| of the module docstring (`roundings` units u per probability)."""
    return roundings * UNIT[dt] * weight + (length * TINY[dt] * vmax).unsqueeze(1) \
        + TOL * max(1.0, float(rounded.abs().max()))


_CASES = {}


def case(batch, heads, dk, dv, dt, seed=0):
    """The references of one configuration, computed once and never modified:
    dict(kqv, windows, counts, max, exact, rounded, lse, bound)."""
    key = (batch, heads, dk, dv, dt, seed)
    if key not in _CASES:
        counts, max_nodes = BATCHES[batch]
        kqv = make_kqv(counts, heads, dk, dv, 7000 + 131 * seed + 17 * dk + 3 * dv + heads + len(counts))
        windows = bounds(counts, max_nodes)
        exact = attention64(kqv, windows, heads, dk, dv)[0]
        rounded, lse, weight, length = attention64(kqv, windows, heads, dk, dv, dt)
        n = kqv.shape[0]
        vmax = float(rnd(kqv.reshape(n, heads, -1)[..., 2 * dk:], dt).abs().max())
        _CASES[key] = dict(kqv=kqv, windows=windows, counts=counts, max=max_nodes, exact=exact, rounded=rounded, lse=lse,
                           bound=out_bound(rounded, weight, length, vmax, dt))
    return _CASES[key]


def precondition(c):
    """(max |exact - rounded| / bound, share of the elements of `exact` outside the bound): from the two float64
    references alone."""
    ratio = (c["exact"] - c["rounded"]).abs() / c["bound"]
    return float(ratio.max()), float((ratio > 1.0).double().mean())
