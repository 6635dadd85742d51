"""Test support for the opt-in 16-bit matrix inputs of the GGNN TRAINING step (`matrix_inputs(dt, training=True)`,
csrc/wgrad16.hip, the training forms in csrc/half_gemm.hip): float64 restatements of the weight gradient, the GRU gates
and the backward GEMMs on ROUNDED operands, and case builders.  Reference, bar and margin are those of
tests/half_cases.py (imported, not repeated).  Never imported by the product package.

The bar's floor.  A weight gradient sums over every ROW: where plain fp32 torch on the same rounded operands is itself
more than a quarter of the bar from float64, the bar is max(bar, 4 x that error), as tests/test_gpu_dense_paths.py does
for the fp32 weight gradient; the precondition (the two float64 references are 20 bars apart) is kept against that larger
bar.
"""
import torch

import half_cases as C
from dense_paths import GRAD_TOL

# the fp32 GEMM families of ops.launch_counts(): none of them may launch where the 16-bit nodes take every GEMM
FP32_GEMM_FAMILIES = ("k_stream_linear", "k_stream_linear_ring", "k_stream_gru", "k_stream_gru_ring", "k_wgrad_stream",
                      "k_linear_tlp", "k_gru", "k_edge_wgrad")
TRAIN_FAMILIES = ("half_wgrad", "half_gru_train", "half_linear_add")
WGRAD_SHAPES = ((32, 32), (64, 96), (128, 384), (96, 160))     # (k, n_out)


def grad_bar(want: torch.Tensor) -> float:
    return GRAD_TOL * max(1.0, float(want.abs().max())) if want.numel() else GRAD_TOL


def wgrad64(x, g, dt=None):
    """grad_w [n_out, k] = rnd(g)^T rnd(x) in float64."""
    return C.rnd64(g, dt).t() @ C.rnd64(x, dt)


def floored_bar(rounded64: torch.Tensor, torch32: torch.Tensor) -> float:
    """C.bar(rounded64), or 4 x the error of fp32 torch on the same rounded operands where that is more than a quarter
    of it (module docstring)."""
    bar, ref32 = C.bar(rounded64), C.err(torch32, rounded64)
    return max(bar, 4.0 * ref32) if ref32 > bar / 4 else bar


def wgrad_bar(x, g, dt) -> float:
    xr, gr = x.detach().cpu().to(dt).float(), g.detach().cpu().to(dt).float()
    return floored_bar(wgrad64(x, g, dt), gr.t() @ xr)


def matmul_bar(a, b_t, dt, addend=None) -> float:
    """Bar of rnd(a) rnd(b_t)^T (+ addend): the input-gradient GEMMs."""
    ar, br = a.detach().cpu().to(dt).float(), b_t.detach().cpu().to(dt).float()
    t32 = ar @ br.t() + (addend.detach().cpu() if addend is not None else 0)
    want = C.rnd64(a, dt) @ C.rnd64(b_t, dt).t() + (addend.detach().cpu().double() if addend is not None else 0)
    return floored_bar(want, t32)


def check(got, rounded, exact, bar, what):
    """The precondition on the inputs (from the two float64 references alone), then the two assertions on the result."""
    gap = C.err(exact, rounded)
    e, e_exact = C.err(got, rounded), C.err(got, exact)
    print(f"  {what}: bar {bar:.3e} gap {gap:.3e} |got - rounded| {e:.3e} |got - exact| {e_exact:.3e}")
    assert gap >= C.MARGIN * bar, f"{what}: inputs do not tell the references apart ({gap:.3e} < 20 x {bar:.3e})"
    assert e <= bar, f"{what}: {e:.3e} > {bar:.3e}"
    assert e_exact >= gap - bar, what


def wgrad_integer_case(rows, k, n_out, seed):
    """x in [-8, 8], g in [-2, 2], integers (the ranges of C.integer_case): every product is at most 16 and every
    partial sum over at most 2 x 512 + 17 rows below 2^15, far below 2^24 -- exact in bf16, fp16 and fp32 in any
    order.  Returns (x, g)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (rows, k), generator=gen).float()
    g = torch.randint(-2, 3, (rows, n_out), generator=gen).float()
    return x, g


def wgrad_exact(x, g):
    return (g.double().t() @ x.double()).float(), g.double().sum(dim=0).float()


def wgrad_random_case(rows, k, n_out, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(rows, k, generator=gen), torch.randn(rows, n_out, generator=gen)


def strided_nan(t: torch.Tensor, left: int, right: int) -> torch.Tensor:
    """`t` as a column slice of a wider CUDA buffer that holds NaN everywhere else (tests/test_gpu_dense_paths.py)."""
    rows, cols = t.shape
    buf = torch.full((rows, left + cols + right), float("nan"), device="cuda")
    buf[:, left:left + cols] = t
    return buf[:, left:left + cols]


def gates64(a, h, w_ih, w_hh, b_ih, b_hh, dt=None):
    """The gates row of the training cell in float64 on rounded operands: [n, 4 hd] = r | z | n | gh_n (gh_n with its
    bias, as ptgnn_amd_gru_cell_backward_gates_f32 reads it)."""
    gi = C.rnd64(a, dt) @ C.rnd64(w_ih, dt).t() + b_ih.detach().cpu().double()
    gh = C.rnd64(h, dt) @ C.rnd64(w_hh, dt).t() + b_hh.detach().cpu().double()
    hd = h.shape[1]
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
    return torch.cat([r, z, n, gh[:, 2 * hd:]], dim=1)

