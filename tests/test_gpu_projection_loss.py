"""The copying decoder's score-free loss on the MI355X (csrc/projection_loss.hip): the two entry points against float64
restatements at every row-block, column-tile and column-chunk boundary, their -inf / out-of-range / determinism rules,
that no [R, V] buffer exists, GruCopyingDecoder.score_free_loss against `fused_loss` and the decoder's reference fixtures,
and Graph2SeqModule with the route switched on.

Boundaries: TR = 64 rows per workgroup, 32-column score tiles, C = 256 forward columns, 1024 row-side backward columns."""
import pytest
import torch

import decoder_cases
import graph2seq_cases
from ptgnn_amd import _lib, ops
from test_gpu_decoder import FIXTURE_TOL, close, no_vendor_calls
from test_gpu_vocab_loss import attributed, decoder_module, grads_of, graph2seq_module, live_inputs, to_dev

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
INF = float("inf")
TR, TILE, C, BWD = 64, 32, 256, 1024
ROWS = [1, TR - 1, TR + 1, 2 * TR + 3]
VOCABS = [1, 31, 33, C - 1, C + 1, 2 * C + 5]
DIMS = [4, 36, 64, 256]
EXTRA_MODES = ("null", "finite", "neg_inf", "plus50")
BIAS_MODES = ("finite", "null", "neg_inf")
GRAD_MODES = ("both", "no_g_norm", "no_g_picked")
# a diagonal through (R, V, E), twice with another offset, so every value of each axis meets several of the others
DIAGONAL = [(ROWS[(i + o) % 4], V, DIMS[(i + 2 * o) % 4], i + 6 * o) for o in (0, 1) for i, V in enumerate(VOCABS)]


def boundary_targets(V, R, shift):
    # 0, V - 1 and both sides of every 32 / 256 / 1024 column boundary below V, starting at `shift`
    marks = sorted({c for b in (TILE, 2 * TILE, C, 2 * C, BWD, 2 * BWD) for c in (b - 1, b) if c < V} | {0, V - 1})
    return torch.tensor([marks[(shift + r) % len(marks)] for r in range(R)], dtype=torch.int64, device=DEV)


def case(R, V, E, run, spread=False):
    """Operands of one call; `run` picks the row padding, the bias / extra / gradient modes and the targets' start."""
    g = torch.Generator().manual_seed(100 * V + 10 * R + E + run)
    pad_p, pad_t = (0, 3)[run % 2], (0, 5)[(run // 2) % 2]
    p = (torch.randn(R, E + pad_p, generator=g) * (40.0 / E ** 0.5 if spread else 1.0)).to(DEV)[:, :E]
    table = torch.randn(V, E + pad_t, generator=g).to(DEV)[:, :E]
    targets = boundary_targets(V, R, run)
    bias_mode, extra_mode, grad_mode = BIAS_MODES[run % 3], EXTRA_MODES[run % 4], GRAD_MODES[(run // 2) % 3]
    bias = torch.randn(V, generator=g).to(DEV) if bias_mode != "null" else None
    if bias_mode == "neg_inf" and V >= TILE - 1:
        keep = bias[targets].clone()
        bias[2::7] = -INF                                               # whole scores of -inf inside live tiles
        bias[targets] = keep
    extra = None
    if extra_mode != "null":
        full = p.double() @ table.double().t() + (bias.double() if bias is not None else 0.0)
        lse = torch.logsumexp(full, dim=-1)
        extra = (lse + torch.randn(R, generator=g).to(DEV).double() * 2.0).float()
        if extra_mode == "neg_inf":
            extra[::3] = -INF
        if extra_mode == "plus50":
            extra[R - 1] = float(lse[R - 1]) + 50.0
    g_norm = torch.randn(R, generator=g).to(DEV) if grad_mode != "no_g_norm" else None
    g_picked = torch.randn(R, generator=g).to(DEV) if grad_mode != "no_g_picked" else None
    return p, table, bias, extra, targets, g_norm, g_picked


def restate(p, table, bias, extra, targets, g_norm, g_picked, dt):
    pp, tt, b, e = [t.detach().to(dt).clone().requires_grad_(True) if t is not None else None for t in (p, table, bias, extra)]
    full = pp @ tt.t() + (b if b is not None else 0.0)
    norm = torch.logsumexp(full, dim=-1)
    if e is not None:
        norm = torch.logaddexp(norm, e)
    picked = full.gather(1, targets.unsqueeze(1)).squeeze(1) - norm
    objective = (norm * g_norm.to(dt)).sum() if g_norm is not None else 0.0
    if g_picked is not None:
        objective = objective + (picked * g_picked.to(dt)).sum()
    d_full, = torch.autograd.grad(objective, full, retain_graph=True)
    objective.backward()
    out = {"norm": norm.detach(), "picked": picked.detach(), "d_projected": pp.grad, "d_table": tt.grad,
           "d_bias": d_full.sum(0)}                                     # the column sum, bias or not
    if e is not None:
        out["d_extra"] = e.grad
    return out


def run_entries(p, table, bias, extra, targets, g_norm, g_picked):
    norm, picked, stats = ops.projection_loss(p, table, bias, extra, targets)
    assert torch.equal(stats.sum(-1), norm)
    d_p, d_table, d_bias, d_extra = ops.projection_loss_backward(p, table, bias, extra, targets, stats, g_norm, g_picked)
    out = {"norm": norm, "picked": picked, "d_projected": d_p, "d_table": d_table, "d_bias": d_bias}
    if extra is not None:
        out["d_extra"] = d_extra
    return out


def check_against_float64(R, V, E, run, spread=False):
    operands = case(R, V, E, run, spread)
    p, table, bias, extra = operands[:4]
    assert (p.stride(0) == E + (0, 3)[run % 2] or R == 1) and (table.stride(0) == E + (0, 5)[(run // 2) % 2] or V == 1)
    before = ops.launch_counts(projection_loss=True)
    got = run_entries(*operands)
    assert ops.launches_since(before) == {"projection_loss": 1, "projection_loss_backward": 1}
    what = f"R={R} V={V} E={E} run={run} spread={spread}"
    res = {dt: restate(*operands, dt) for dt in (torch.float32, torch.float64)}
    if spread and V >= TILE - 1:
        full = p.double() @ table.double().t() + (bias.double() if bias is not None else 0.0)
        assert float((full.max(-1)[0] - full.min(-1)[0]).max()) > 100.0   # exp overflows without the running maximum
    assert sorted(got) == sorted(res[torch.float64])
    for k, val in got.items():
        assert bool(torch.isfinite(val).all()), (what, k)
        assert attributed(val, res[torch.float32][k], res[torch.float64][k], f"{what} {k}"), (what, k)
    if extra is not None and bool((extra == -INF).any()):               # the vocabulary term bit for bit, exact zeros
        rows = extra == -INF
        assert torch.equal(got["norm"][rows], ops.projection_loss(p, table, bias, None, operands[4])[0][rows])
        assert float(got["d_extra"][rows].abs().max()) == 0.0


# the diagonal, the reference vocabulary, and scores that span more than 100
CASES = [c + (False,) for c in DIAGONAL + [(14, 20000, 64, r) for r in (0, 5, 10)]] \
    + [(TR + 1, 33, 36, 3, True), (2 * TR + 3, 2 * C + 5, 256, 4, True), (14, 20000, 64, 7, True)]


@pytest.mark.parametrize("R,V,E,run,spread", CASES)
def test_projection_loss_and_backward_against_float64(R, V, E, run, spread):
    check_against_float64(R, V, E, run, spread)


def test_edge_rules_of_targets_and_empty_states():
    operands = case(TR + 1, C + 1, 36, 1)
    p, table, bias, extra, targets, g_norm, g_picked = operands
    good = run_entries(*operands)
    row, keep = 2, torch.arange(TR + 1, device=DEV) != 2
    for bad_value in (C + 1, -1, 2 ** 40):
        bad_targets = targets.clone()
        bad_targets[row] = bad_value
        bad = run_entries(p, table, bias, extra, bad_targets, g_norm, g_picked)
        assert bool(torch.isnan(bad["picked"][row])) and torch.equal(bad["picked"][keep], good["picked"][keep])
        assert torch.equal(bad["norm"], good["norm"]) and torch.equal(bad["d_projected"][keep], good["d_projected"][keep])
        for k in ("d_projected", "d_table", "d_bias", "d_extra"):
            assert bool(torch.isfinite(bad[k]).all()), k                # the bad row has no picked entry: softmax term only
    # the (-inf, 0) state of softmax_state.h: a row whose every score is -inf, alone and under a finite copy term
    empty_bias = torch.full((C + 1,), -INF, device=DEV)
    norm, _, stats = ops.projection_loss(p, table, empty_bias)
    assert bool((norm == -INF).all()) and stats[0].tolist() == [-INF, 0.0]
    copy = torch.randn(TR + 1, device=DEV)
    assert torch.equal(ops.projection_loss(p, table, empty_bias, copy)[0], copy)


def test_two_calls_and_padded_rows_give_the_same_bits():
    for R, V, E, run in ((14, 20000, 64, 3), (2 * TR + 3, 2 * C + 5, 36, 3)):
        operands = case(R, V, E, run, spread=True)
        assert operands[0].stride(0) != E and operands[1].stride(0) != E
        first, second = run_entries(*operands), run_entries(*operands)
        packed = run_entries(operands[0].contiguous(), operands[1].contiguous(), *operands[2:])
        for k in first:
            assert torch.equal(first[k], second[k]) and torch.equal(first[k], packed[k]), (V, k)


def test_no_buffer_of_rows_times_vocabulary_exists():
    R, V, E = 512, 8192, 32
    lib = _lib.load()
    documented = 8 * R * ((V + C - 1) // C) + 4 * R + 4 * ((V + BWD - 1) // BWD) * R * E
    assert lib.ptgnn_amd_projection_loss_workspace_bytes(R, V) \
        + lib.ptgnn_amd_projection_loss_backward_workspace_bytes(R, V, E) <= documented + 3 * 256 < R * V * 4 // 16
    operands = case(R, V, E, 0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    got = run_entries(*operands)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - held
    assert rise < R * V * 4 // 2 and bool(torch.isfinite(got["d_table"]).all())


def score_free_run(module, fx, seed=None):
    module.zero_grad(set_to_none=True)
    inputs = live_inputs(fx)
    if seed is not None:
        torch.manual_seed(seed)
    before = ops.launch_counts(sequence=True, projection_loss=True)
    with no_vendor_calls():
        loss = module.score_free_loss(**inputs)
        loss.backward()
    ran = ops.launches_since(before)
    assert {k: ran.get(k, 0) for k in ("projection_loss", "projection_loss_backward", "vocab_loss", "copy_loss_finish")} \
        == {"projection_loss": 1, "projection_loss_backward": 1, "vocab_loss": 0, "copy_loss_finish": 1}, ran
    return loss.detach().clone(), {k: g.clone() for k, g in grads_of(module, inputs).items()}


@pytest.mark.parametrize("name,spec", decoder_cases.CASES, ids=[n for n, _ in decoder_cases.CASES])
def test_score_free_loss_against_fused_loss_and_the_reference_fixture(name, spec):
    fx, module = decoder_module(name, spec)
    loss, grads = score_free_run(module, fx)
    assert close(loss, fx["loss"])
    for k, g in grads.items():
        assert close(g, fx["grad." + k]), k
    module.zero_grad(set_to_none=True)
    inputs = live_inputs(fx)
    fused = module.fused_loss(**inputs)
    fused.backward()
    assert close(loss, fused, 1e-5)
    for k, g in grads_of(module, inputs).items():
        assert close(grads[k], g, FIXTURE_TOL), k


def test_score_free_loss_of_a_dropout_module():
    name, spec = decoder_cases.CASES[0]
    fx, module = decoder_module(name, spec, 0.2)
    module.train()
    runs = [score_free_run(module, fx, seed) for seed in (5, 5, 6)]
    assert torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], runs[2][0])
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]) and bool(torch.isfinite(g).all()), k
    assert bool(torch.isfinite(runs[0][0])) and bool(torch.isfinite(runs[2][0]))


def test_graph2seq_module_with_the_score_free_route():
    name, spec = graph2seq_cases.CASES[0]
    fx, module = graph2seq_module(name, spec)
    inputs = graph2seq_cases.inputs_of(fx)
    before = ops.launch_counts(projection_loss=True)
    with torch.no_grad():
        module(**graph2seq_cases.call_args(spec, inputs, to=to_dev))    # the default route
    assert not {"projection_loss", "projection_loss_backward"} & set(ops.launches_since(before))
    module.use_score_free_loss = True
    states = tuple(inputs[k].to(DEV).requires_grad_(True) for k in ("input_states", "output_states"))
    with no_vendor_calls():
        loss = module(**graph2seq_cases.call_args(spec, inputs, to=to_dev, states=states))
        loss.backward()
    ran = ops.launches_since(before)
    assert (ran.get("projection_loss"), ran.get("projection_loss_backward")) == (1, 1)
    assert close(loss, fx["loss"])
    assert close(states[0].grad, fx["grad.input_states"]) and close(states[1].grad, fx["grad.output_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k
