"""The score-free loss with 16-bit matrix-core inputs on the MI355X (csrc/projection_loss16.hip): the two entries against
float64 on the rounded operands, the rules of the fp32 pair that must survive, and the decoder under its switch."""
import pytest
import torch

import decoder_cases
import ptgnn_amd
from ptgnn_amd import ops
from test_gpu_projection_loss import DIMS, INF, ROWS, case, restate
from test_gpu_vocab_loss import attributed, decoder_module, grads_of, live_inputs

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
COUNTERS = dict(projection_loss=True, projection_loss16=True)
ONLY16 = {"projection_loss16": 1, "projection_loss16_backward": 1}
# the fp32 file's diagonal through (R, V, E) with a last vocabulary past the 1024-column chunk of the row-side backward: two
# partials of d_projected to fold, d_extra from chunk 0 alone, targets on both sides of 1024
VOCABS = [1, 31, 33, 255, 257, 1029]
DIAGONAL = [(ROWS[(i + o) % 4], V, DIMS[(i + 2 * o) % 4], i + 6 * o) for o in (0, 1) for i, V in enumerate(VOCABS)]


def run_entries(operands, dt):
    p, table, bias, extra, targets, g_norm, g_picked = operands
    norm, picked, stats = ops.projection_loss(p, table, bias, extra, targets, inputs=dt)
    d_p, d_table, d_bias, d_extra = ops.projection_loss_backward(p, table, bias, extra, targets, stats, g_norm, g_picked,
                                                                 inputs=dt)
    out = {"norm": norm, "picked": picked, "d_projected": d_p, "d_table": d_table, "d_bias": d_bias}
    if extra is not None:
        out["d_extra"] = d_extra
    return out


def score_gradient(p, table, bias, extra, targets, g_norm, g_picked):
    """G [R, V] in float64: the derivative of the objective of `restate` with respect to the scores."""
    full = (p.double() @ table.double().t() + (bias.double() if bias is not None else 0.0)).requires_grad_(True)
    norm = torch.logsumexp(full, dim=-1)
    if extra is not None:
        norm = torch.logaddexp(norm, extra.double())
    picked = full.gather(1, targets.unsqueeze(1)).squeeze(1) - norm
    objective = (norm * g_norm.double()).sum() if g_norm is not None else 0.0
    if g_picked is not None:
        objective = objective + (picked * g_picked.double()).sum()
    return torch.autograd.grad(objective, full)[0]


def check_against_float64(R, V, E, run, dt, spread=False):
    operands = case(R, V, E, run, spread)
    p, table = operands[:2]
    rounded = (p.to(dt).float(), table.to(dt).float()) + operands[2:]
    before = ops.launch_counts(**COUNTERS)
    got = run_entries(operands, dt)
    assert ops.launches_since(before) == ONLY16
    what = f"R={R} V={V} E={E} run={run} {dt} spread={spread}"
    res = {t: restate(*rounded, t) for t in (torch.float32, torch.float64)}
    assert sorted(got) == sorted(res[torch.float64])
    for k, val in got.items():
        assert bool(torch.isfinite(val).all()), (what, k)
    for k in set(got) - {"d_projected", "d_table"}:       # only the fp32 accumulation separates these from the restatement
        assert attributed(got[k], res[torch.float32][k], res[torch.float64][k], f"{what} {k}"), (what, k)
    if E >= 36:                           # the inputs tell the rounded operands from the unrounded ones
        plain = ops.projection_loss(*operands[:5])[0].double()
        exact, ref32 = res[torch.float64]["norm"], res[torch.float32]["norm"].double()
        bar = max(1e-5 * max(1.0, float(exact.abs().max())), 2.0 * float((ref32 - exact).abs().max()))
        assert float((plain - exact).abs().max()) >= 2.0 * bar, what
    # the gradient products: one rounding of G against the rounded operand, n fp32 additions
    u, G = UNIT[dt], score_gradient(*rounded).abs()
    for k, mass, operand, n in (("d_projected", G, rounded[1], V), ("d_table", G.t(), rounded[0], R)):
        bound = (u + (n + 2) * 2.0 ** -24) * (mass @ operand.double().abs())
        if dt == torch.float16:                            # entries of G below the fp16 normal range
            bound = bound + 2.0 ** -25 * operand.double().abs().sum(0)
        err = (got[k].double() - res[torch.float64][k]).abs()
        print(f"    {what} {k}: max |error| / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (what, k)
    return operands, got


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("R,V,E,run", DIAGONAL)
def test_entries_against_float64_on_the_rounded_operands(R, V, E, run, dt):
    check_against_float64(R, V, E, run, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_rules_that_survive_the_16_bit_path(dt):
    R, V, E, run = 65, 257, 36, 2                          # bias and extra with -inf entries, padded table rows
    operands, first = check_against_float64(R, V, E, run, dt)
    p, table, bias, extra, targets = operands[:5]
    second = run_entries(operands, dt)
    moved = [torch.zeros(t.shape[0], E + 7, device=t.device)[:, 1:E + 1].copy_(t) for t in (p, table)]
    assert moved[0].data_ptr() % 16 == 4 and moved[0].stride(0) != p.stride(0)
    shifted = run_entries(tuple(moved) + operands[2:], dt)
    for k in first:
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], shifted[k]), k
    rows, cols = extra == -INF, bias == -INF
    assert bool(rows.any()) and bool(cols.any())
    assert torch.equal(first["norm"][rows], ops.projection_loss(p, table, bias, None, targets, inputs=dt)[0][rows])
    assert float(first["d_extra"][rows].abs().max()) == 0.0
    assert float(first["d_table"][cols].abs().max()) == 0.0
    check_against_float64(R, V, E, run, dt, spread=True)   # scores that span more than 100


def decoder_run(module, fx, loss_of, expect):
    module.zero_grad(set_to_none=True)
    inputs = live_inputs(fx)
    before = ops.launch_counts(**COUNTERS)
    loss = loss_of(module)(**inputs)
    loss.backward()
    assert {k: n for k, n in ops.launches_since(before).items() if k.startswith("projection_loss")} == expect
    grads = grads_of(module, inputs)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    return [loss.detach().clone()] + [grads[k].clone() for k in sorted(grads)]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_the_decoder_under_the_switch(dt, monkeypatch):
    name, spec = decoder_cases.CASES[0]
    fx, module = decoder_module(name, spec)
    only32 = {"projection_loss": 1, "projection_loss_backward": 1}
    score_free, fused = (lambda m: m.score_free_loss), (lambda m: m.fused_loss)
    plain, plain_fused = decoder_run(module, fx, score_free, only32), decoder_run(module, fx, fused, {})
    seen = []
    entry = ops.projection_loss
    monkeypatch.setattr(ops, "projection_loss",
                        lambda p, t, *a, **kw: seen.append((p.detach(), t.detach())) or entry(p, t, *a, **kw))
    with ptgnn_amd.vocabulary_loss(), ptgnn_amd.matrix_inputs(dt):
        assert ptgnn_amd.vocabulary_loss_inputs(plain[0]) == dt
        half = decoder_run(module, fx, score_free, ONLY16)
        for a, b in zip(plain_fused, decoder_run(module, fx, fused, {})):
            assert torch.equal(a, b)
    with ptgnn_amd.matrix_inputs(dt):                      # the dtype setting alone leaves the decoder alone
        for a, b in zip(plain, decoder_run(module, fx, score_free, only32)):
            assert torch.equal(a, b)
    # every score moves by at most (2 u + u^2) A; everything behind the scores is 1-Lipschitz in the sup norm, twice
    p, table = seen[0]
    A, u = float((p.double().abs() @ table.double().abs().t()).max()), UNIT[dt]
    print(f"    {dt}: |loss16 - loss32| = {float((half[0] - plain[0]).abs()):.3e}, A = {A:.3e}")
    assert float((half[0] - plain[0]).abs()) <= 2.0 * (2.0 * u + u * u) * A + 1e-5
