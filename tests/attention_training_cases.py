"""Cases and float64 restatements for the 16-bit attention TRAINING step (`ptgnn_amd.set_attention_training`;
csrc/block_attention16.hip with dropout, csrc/block_attention16_backward.hip).  Support for
tests/test_attention_training.py and tests/test_gpu_attention_training.py; never imported by the package.

Two restatements of selfattmessagepassing.py:104-117 and its autograd per window and head, both float64, M the dropout
multiplier (1 / (1 - p) or 0; ones without dropout), s = 1 / sqrt(dk):

    exact     k, q, v, dOut as they are
    rounded   k, q, v, dOut rounded to the 16-bit type where they enter a product; P, M o P and dS UNROUNDED:
              P = softmax(s rnd(K) rnd(Q)^T), out = (M o P) rnd(V), D = sum_d dOut o out (dOut unrounded),
              dP = rnd(dOut) rnd(V)^T, dS = P o (M o dP - D),
              dK = s dS rnd(Q), dQ = s dS^T rnd(K), dV = (M o P)^T rnd(dOut)

The kernels differ from `rounded` by four things only (u = 2^-8 bf16 / 2^-11 fp16, tiny = 2^-25 for fp16, n = rows of the
window, TOL the bar of tests/dense_paths.py):
  1. one rounding of each M o P and each dS: at most u relative, plus tiny absolute (fp16 gradual underflow);
  2. the forward's own `out` inside D, which carries the forward bound of tests/attention_inputs_cases.py with M o P for P:
     |dD_k| <= sum_d |dOut_kd| (u ((M o P) |rnd V|)_kd + n tiny max|rnd V| + TOL max(1, |out|max)) =: E_k,
     and dS moves by at most P_kv E_k;
  3. fp32 arithmetic: TOL max(1, |reference|max) per slice.
So, elementwise,
    |d out| <= u ((M o P) |rnd V|) + n tiny max|rnd V| + TOL max(1, |out|max)
    |d dV|  <= u ((M o P)^T |rnd dOut|) + n tiny max|rnd dOut| + TOL max(1, |dV|max)
    |d dK|  <= s ((u |dS| + P o E) |rnd Q| + n tiny max|rnd Q|) + TOL max(1, |dK|max)
    |d dQ|  <= s ((u |dS| + P o E)^T |rnd K| + n tiny max|rnd K|) + TOL max(1, |dQ|max)
The bounds are derived, never fitted to what the kernels give."""
import math

import torch

import attention_inputs_cases as A
from attention_inputs_cases import TINY, UNIT, attention64, bounds, make_kqv  # noqa: F401  (attention64: the p = 0 forward)
from dense_paths import TOL
from helpers import dropout_keep_scale

BATCHES = dict(A.BATCHES, w161=([161], 250))       # 161 = 128 + 33: a second row block with one full and one 1-row wave
# (batch, heads, dk, dv, p, max_num_nodes override or None): a cross-section of batches x widths x heads x dropout
CASES = [("max33", 3, 32, 32, 0.0, None), ("max33", 1, 17, 6, 0.25, None), ("w97", 3, 64, 128, 0.0, None),
         ("w97", 1, 128, 64, 0.25, None), ("w161", 1, 32, 32, 0.25, None), ("w161", 3, 17, 6, 0.0, None),
         ("max33", 3, 1, 1, 0.0, None), ("max33", 3, 32, 32, 0.25, 31)]     # the last: odd max_num_nodes, mask width 32
# (dk = dv = 1 sits on the short windows: in a 97- or 161-row window its two references are less than a bound apart)
SEED = (7 << 40) + 4321


def case_id(c):
    return f"{c[0]}-h{c[1]}k{c[2]}v{c[3]}p{c[4]}" + (f"-max{c[5]}" if c[5] else "")


def step64(kqv, gout, windows, heads, dk, dv, keep, dt=None):
    """float64 forward and backward of the module docstring; dt None = `exact`, else `rounded`.  `keep`: the [N heads, W]
    multiplier (row r heads + h, column = position in the window) or None.
    -> dict(out, grad) and, for `rounded`, the elementwise bounds dict(out_bound, grad_bound)."""
    n, hw = kqv.shape[0], 2 * dk + dv
    r = (lambda t: t.to(dt).double()) if dt is not None else (lambda t: t.double())
    x, g, gr = r(kqv).reshape(n, heads, hw), gout.double().reshape(n, heads, dv), r(gout).reshape(n, heads, dv)
    u, tiny = (UNIT[dt], TINY[dt]) if dt is not None else (0.0, 0.0)
    s = 1.0 / math.sqrt(dk)
    out, grad = torch.zeros(n, heads, dv, dtype=torch.float64), torch.zeros(n, heads, hw, dtype=torch.float64)
    out_b, grad_b = torch.zeros_like(out), torch.zeros_like(grad)
    parts = []
    for lo, hi in windows:
        k, q, v = x[lo:hi, :, :dk], x[lo:hi, :, dk:2 * dk], x[lo:hi, :, 2 * dk:]
        p = torch.softmax(torch.einsum("khd,vhd->khv", k, q) * s, dim=-1)
        m = torch.ones_like(p) if keep is None else \
            keep.reshape(n, heads, -1)[lo:hi, :, :hi - lo].double()
        mp = m * p
        out[lo:hi] = torch.einsum("khv,vhd->khd", mp, v)
        d = (g[lo:hi] * out[lo:hi]).sum(-1, keepdim=True)
        ds = p * (m * torch.einsum("khd,vhd->khv", gr[lo:hi], v) - d)
        grad[lo:hi, :, :dk] = s * torch.einsum("khv,vhd->khd", ds, q)
        grad[lo:hi, :, dk:2 * dk] = s * torch.einsum("khv,khd->vhd", ds, k)
        grad[lo:hi, :, 2 * dk:] = torch.einsum("khv,khd->vhd", mp, gr[lo:hi])
        parts.append((lo, hi, k, q, v, p, mp, ds))
    if dt is None:
        return dict(out=out.reshape(n, -1), grad=grad.reshape(n, -1))
    bar_out = TOL * max(1.0, float(out.abs().max()))
    bars = [TOL * max(1.0, float(grad[..., a:b].abs().max())) for a, b in ((0, dk), (dk, 2 * dk), (2 * dk, hw))]
    for lo, hi, k, q, v, p, mp, ds in parts:
        w = hi - lo
        out_b[lo:hi] = u * torch.einsum("khv,vhd->khd", mp, v.abs()) + w * tiny * float(v.abs().max()) + bar_out
        e = (g[lo:hi].abs() * out_b[lo:hi]).sum(-1, keepdim=True)                  # E_k
        moved = u * ds.abs() + p * e
        grad_b[lo:hi, :, :dk] = s * (torch.einsum("khv,vhd->khd", moved, q.abs()) + w * tiny * float(q.abs().max())) \
            + bars[0]
        grad_b[lo:hi, :, dk:2 * dk] = s * (torch.einsum("khv,khd->vhd", moved, k.abs())
                                           + w * tiny * float(k.abs().max())) + bars[1]
        grad_b[lo:hi, :, 2 * dk:] = u * torch.einsum("khv,khd->vhd", mp, gr[lo:hi].abs()) \
            + w * tiny * float(gr[lo:hi].abs().max()) + bars[2]
    return dict(out=out.reshape(n, -1), grad=grad.reshape(n, -1), out_bound=out_b.reshape(n, -1),
                grad_bound=grad_b.reshape(n, -1))


_CASES = {}


def case(c, dt):
    """The references of one entry of CASES, computed once and never modified:
    dict(kqv, gout, counts, max, windows, keep, exact, rounded)."""
    key = (c, dt)
    if key not in _CASES:
        batch, heads, dk, dv, p, max_nodes = c
        counts = BATCHES[batch][0]
        max_nodes = max_nodes or BATCHES[batch][1]
        kqv = make_kqv(counts, heads, dk, dv, 9100 + 17 * dk + 3 * dv + heads + len(counts))
        gout = torch.randn(kqv.shape[0], heads * dv, generator=torch.Generator().manual_seed(9200 + dk + dv))
        windows = bounds(counts, max_nodes)
        keep = dropout_keep_scale(SEED, kqv.shape[0] * heads, (max_nodes + 1) // 2 * 2, p) if p > 0 else None
        _CASES[key] = dict(kqv=kqv, gout=gout, counts=counts, max=max_nodes, windows=windows, keep=keep,
                           exact=step64(kqv, gout, windows, heads, dk, dv, keep),
                           rounded=step64(kqv, gout, windows, heads, dk, dv, keep, dt))
    return _CASES[key]


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements."""
    return float(((got.double() - ref).abs() / bound).max())
