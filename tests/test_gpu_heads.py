"""The task heads on the MI355X (csrc/task_heads.hip, ptgnn_amd/heads.py): the three modules against the reference
fixtures, without vendor calls and without a blocking read, the two kernels against float64 restatements at every width
class and chunk boundary, determinism, the composed route beyond the candidate kernel's range, AMP dtypes and empty inputs."""
import contextlib
import math
from unittest import mock

import pytest
import torch
from torch import nn

from agg_paths import TOL, attributed_ok
from head_cases import ALL_HEAD_CASES, LFE_CASES, StubGnn, build, build_lfe, call_args, inputs_of, load, state_of
from ptgnn_amd import embeddings, heads, ops
from ptgnn_amd.gnn import GnnOutput
from segment_batches import candidate_ref, sigmoid_ref, softmax_ref, softmax_targets

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXTURE_TOL = 2e-5          # the bar of tests/test_decoder_cpu.py, relative to max(1, max |want|)
IDS = [name for _, name, _ in ALL_HEAD_CASES]
INF = float("inf")
FAMILIES = {"g2c": ("logit_loss", "logit_loss_backward"), "ppi": ("logit_loss", "logit_loss_backward"),
            "vm": ("candidate_scores", "candidate_scores_backward")}


def close(got, want, tol=FIXTURE_TOL):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).double().cpu()
    if got.shape != want.shape:
        return False
    err, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
    print(f"    |got - want| = {err:.3e} (scale {scale:.3e})")
    return err <= tol * scale


def attributed(got, want32, exact, what=""):
    """agg_paths.attributed_ok relative to max(1, max |float64|); -inf entries must sit at the same positions."""
    got, want32, exact = (t.detach().double().cpu() for t in (got, want32, exact))
    assert torch.equal(got == -INF, exact == -INF), what
    finite = torch.isfinite(exact)
    if not bool(finite.any()):
        return True
    got, want32, exact = got[finite], want32[finite], exact[finite]
    scale = max(1.0, float(exact.abs().max()))
    print(f"    {what}: |got-fp32|={float((got - want32).abs().max()):.3e} |got-f64|={float((got - exact).abs().max()):.3e} "
          f"scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


def _refuse(name):
    def raiser(*args, **kwargs):
        raise AssertionError(f"{name} was called on the GPU route")
    return raiser


@contextlib.contextmanager
def no_vendor_calls():
    with mock.patch.object(nn.functional, "linear", _refuse("F.linear")), \
            mock.patch.object(nn.functional, "cross_entropy", _refuse("F.cross_entropy")), \
            mock.patch.object(nn.functional, "binary_cross_entropy_with_logits", _refuse("F.bce_with_logits")), \
            mock.patch.object(torch, "cat", _refuse("torch.cat")):
        yield


@contextlib.contextmanager
def no_blocking_reads():
    """Every way a CUDA tensor's value reaches Python raises."""
    def guard(name):
        real = getattr(torch.Tensor, name)

        def guarded(self, *args, **kwargs):
            if self.is_cuda:
                raise AssertionError(f"Tensor.{name} of a CUDA tensor: a blocking read")
            return real(self, *args, **kwargs)
        return mock.patch.object(torch.Tensor, name, guarded)

    with contextlib.ExitStack() as stack:
        for name in ("item", "tolist", "cpu", "__int__", "__float__", "__bool__"):
            stack.enter_context(guard(name))
        yield


def fixture_module(kind, name, spec):
    fx = load(name)
    module = build(kind, spec, heads, GnnOutput)
    module.load_state_dict(state_of(fx), strict=True)
    return fx, module.to(DEV)


def to_dev(t):
    return t.to(DEV)


def check_against_fixture(kind, fx, module, inputs, guard):
    """forward + backward of the first minibatch, forward of the second, predict: everything the fixture holds."""
    module.reset_metrics()
    states = inputs["node_states"].to(DEV).requires_grad_(True)
    with guard():
        predicted = module.predict(call_args(kind, inputs, to=to_dev)[0]) if kind == "g2c" else None
        loss = module(*call_args(kind, inputs, to=to_dev, states=states))
        loss.backward()
    first = module.report_metrics()
    with guard(), torch.no_grad():
        second_loss = module(*call_args(kind, inputs, second=True, to=to_dev))
    second = module.report_metrics()
    assert loss.dtype == torch.float32 and close(loss, fx["loss"]) and close(second_loss, fx["second.loss"])
    assert close(states.grad, fx["grad.node_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k
    for tag, got in (("metrics1.", first), ("metrics2.", second)):
        assert sorted(tag + k for k in got) == sorted(k for k in fx if k.startswith(tag))
        for k, v in got.items():
            if k == "Accuracy":
                assert float(v) == float(fx[tag + k]), (tag, k, v)        # a ratio of two integer counts: exact
            else:
                assert close(float(v), fx[tag + k]), (tag, k)
    if predicted is not None:
        probs, classes, graph_idx = predicted
        assert close(probs, fx["predict.probs"])
        assert torch.equal(classes.cpu(), torch.from_numpy(fx["predict.classes"]))
        assert torch.equal(graph_idx.cpu(), torch.from_numpy(fx["predict.graph_idx"]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. - 3. the reference fixtures: values, no vendor call, no blocking read
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_reference_fixtures_on_the_gpu(kind, name, spec):
    fx, module = fixture_module(kind, name, spec)
    check_against_fixture(kind, fx, module, inputs_of(fx), contextlib.nullcontext)


@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_reference_fixtures_without_vendor_calls(kind, name, spec):
    fx, module = fixture_module(kind, name, spec)
    before = ops.launch_counts(heads=True)
    check_against_fixture(kind, fx, module, inputs_of(fx), no_vendor_calls)
    ran = ops.launches_since(before)
    forward, backward = FAMILIES[kind]
    assert ran.get(forward, 0) >= 2 and ran.get(backward, 0) == 1, ran
    for other in set(sum(FAMILIES.values(), ())) - {forward, backward}:
        assert other not in ran, ran


@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES, ids=IDS)
def test_forward_backward_and_predict_never_block_the_host(kind, name, spec):
    fx, module = fixture_module(kind, name, spec)
    check_against_fixture(kind, fx, module, inputs_of(fx), no_blocking_reads)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the logit-loss kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
def check_logit_loss_kernel(R, C, mode, gen):
    """One [R, C] call of `heads.logit_loss` with backward against float64; every integer total and the metrics block exactly
    (shared with tests/test_gpu_many_segments.py, which takes R past one run of chunks per merge thread)."""
    if mode == "softmax":
        logits = ((torch.rand(R, C, generator=gen) - 0.5) * 200.0).to(DEV)          # a spread of 200
        targets = softmax_targets(R, C, gen).to(DEV)
        ref = softmax_ref
    else:
        logits = ((torch.rand(R, C, generator=gen) - 0.5) * 120.0).to(DEV)          # +-60
        targets = (torch.rand(R, C, generator=gen) < 0.4).to(DEV)
        ref = sigmoid_ref
    g = torch.tensor(2.5, device=DEV)                                                # a non-unit upstream scalar
    live_logits = logits.clone().requires_grad_(True)
    metrics = ops.head_metrics_block(DEV)
    before = ops.launch_counts(heads=True)
    loss = heads.logit_loss(live_logits, targets, mode, metrics)
    (loss * g).backward()
    assert ops.launches_since(before) == {"logit_loss": 1, "logit_loss_backward": 1}
    want32, lse32, l32 = ref(logits, targets, torch.float32)
    exact, lse64, l64 = ref(logits, targets, torch.float64)
    (want32 * g).backward()
    (exact * g.double()).backward()
    print(f"  {mode} R={R} C={C}")
    assert attributed(loss, want32, exact, "loss")
    assert attributed(live_logits.grad, l32.grad, l64.grad, "grad_logits")
    _, lse, argmax, max_prob, totals = ops.logit_loss(logits, targets, mode)
    totals = totals.cpu()
    counts = totals.tolist()
    if mode == "softmax":
        assert attributed(lse, lse32, lse64, "lse")
        live = (targets >= 0) & (targets < C)
        assert torch.equal(argmax, logits.argmax(dim=-1))                            # random floats: no ties
        assert attributed(max_prob, (logits.max(-1)[0] - lse32).exp(), (logits.double().max(-1)[0] - lse64).exp(), "max prob")
        assert counts[1:6] == [int(live.sum()), int(((argmax == targets) & live).sum()),
                               int((~live & (targets != -100)).sum()), 0, R]
        assert not bool(live_logits.grad[~live].any())                               # ignored rows: exact zeros
        assert metrics.tolist() == [counts[2], counts[1], counts[3], 0]
    else:
        pred, t = logits >= 0, targets
        tp, fp, fn = int((pred & t).sum()), int((pred & ~t).sum()), int((~pred & t).sum())
        assert counts[1:6] == [R, tp, fp, fn, R]
        tpf, fpf, fnf = (torch.tensor(float(v), dtype=torch.float32) for v in (tp, fp, fn))
        pr, re = tpf / (tpf + fpf + 1e-10), tpf / (tpf + fnf + 1e-10)
        f1 = 2 * pr * re / (pr + re + 1e-10)
        sums = metrics.cpu().view(torch.float64)
        for got, want in zip(sums[:3].tolist(), (pr, re, f1)):
            assert abs(got - float(want) * R) <= 1e-6 * R, (got, float(want) * R)    # fp32 expression: a few ulp of <= 1
        assert int(metrics[3]) == R
    assert float(totals[:1].view(torch.float64)) == pytest.approx(float(exact) * counts[1], rel=1e-5)


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 100, 121, 257, 1025])
def test_logit_loss_kernel_against_float64(C, mode):
    gen = torch.Generator().manual_seed(1000 + C)
    for R in (1, 127, 128, 129, 300):
        check_logit_loss_kernel(R, C, mode, gen)


def test_logit_loss_all_rows_ignored_and_ties():
    logits = torch.randn(5, 7).to(DEV).requires_grad_(True)
    targets = torch.full((5,), -100, dtype=torch.int64)
    loss = heads.logit_loss(logits, targets.to(DEV), "softmax")
    loss.backward()
    cpu = nn.functional.cross_entropy(logits.detach().cpu(), targets)                     # the CPU route's answer: nan
    assert math.isnan(float(cpu)) and math.isnan(float(loss))
    assert not bool(logits.grad.any())                                                    # no gradient anywhere
    tied = torch.zeros(3, 130, device=DEV)
    tied[0, [5, 70]] = 2.0                    # the same lane sees both; two lanes; a lane and the butterfly
    tied[1, [64, 3]] = 2.0
    tied[2, [129, 128, 127]] = 2.0
    _, _, argmax, _, _ = ops.logit_loss(tied, None, "softmax")
    assert argmax.tolist() == [5, 3, 127]                                                 # the lowest index on ties


def test_logit_loss_rows_that_are_or_start_with_minus_infinity():
    """The edge rule of csrc/softmax_state.h for the state with an arg-max: it takes its first element unconditionally, so
    a row of -inf has lse = -inf and its first index as the arg-max, and a leading -inf is forgotten by what follows."""
    logits = torch.tensor([[-INF] * 5, [-INF, 0.5, -1.25, 2.0, 0.25], [0.75, -0.5, 1.5, -2.0, 0.0]])
    _, lse, argmax, _, _ = ops.logit_loss(logits.to(DEV), None, "softmax")
    exact = torch.logsumexp(logits.double(), dim=-1)                                      # on the CPU
    assert exact.tolist()[0] == -INF and bool(torch.isfinite(exact[1:]).all())
    assert torch.equal(torch.isnan(lse.cpu()), torch.isnan(exact))
    assert attributed(lse, torch.logsumexp(logits, dim=-1), exact, "lse")                 # -inf at the same positions
    assert argmax.tolist() == [0, 3, 2]


# ---------------------------------------------------------------------------------------------------------------------
# 5. the candidate kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
SLOT_SIZES = [0, 1, 63, 64, 65, 300]


def candidate_batch(D, gen, N=700):
    """An unsorted candidate -> slot map over SLOT_SIZES, a node that is a candidate twice (in one slot) and a node that is
    both a slot and a candidate; the empty slot's correct index is -1 (skipped and counted)."""
    G, Cn = len(SLOT_SIZES), sum(SLOT_SIZES)
    cand_slot = torch.repeat_interleave(torch.arange(G), torch.tensor(SLOT_SIZES))
    cand_slot = cand_slot[torch.randperm(Cn, generator=gen)]
    cand_idx = torch.randperm(N, generator=gen)[:Cn]
    in3 = torch.nonzero(cand_slot == 3).flatten()
    cand_idx[in3[1]] = cand_idx[in3[0]]                       # twice a candidate
    slot_idx = torch.randint(0, N, (G,), generator=gen)
    slot_idx[2] = cand_idx[in3[2]]                            # both slot and candidate
    correct = torch.tensor([-1 if n == 0 else int(torch.nonzero(cand_slot == g).flatten()[n // 2])
                            for g, n in enumerate(SLOT_SIZES)])
    x = torch.randn(N, D, generator=gen)
    w = torch.randn(1, 2 * D, generator=gen) / math.sqrt(D)
    return x, w, cand_idx, slot_idx, cand_slot, correct


@pytest.mark.parametrize("D", [4, 60, 128, 1024])
def test_candidate_kernel_against_float64(D):
    gen = torch.Generator().manual_seed(2000 + D)
    x, w, cand_idx, slot_idx, cand_slot, correct = (t.to(DEV) for t in candidate_batch(D, gen))
    cot = torch.randn(cand_idx.shape[0], generator=gen).to(DEV)                           # a random dscores
    g = torch.tensor(1.75, device=DEV)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    metrics = ops.head_metrics_block(DEV)
    before = ops.launch_counts(heads=True)
    loss, scores, lse, argmax = heads.candidate_loss(xl, wl, cand_idx, slot_idx, cand_slot, correct, metrics)
    (loss * g + (scores * cot).sum()).backward()
    assert ops.launches_since(before) == {"candidate_scores": 1, "candidate_scores_backward": 1}
    r32 = candidate_ref(x, w, cand_idx, slot_idx, cand_slot, correct, cot, g, torch.float32)
    r64 = candidate_ref(x, w, cand_idx, slot_idx, cand_slot, correct, cot, g, torch.float64)
    assert attributed(loss, r32[0], r64[0], "loss")
    assert attributed(scores, r32[1], r64[1], "scores")
    assert attributed(lse, r32[2], r64[2], "lse")
    assert float(lse[0]) == -INF and int(argmax[0]) == cand_idx.shape[0]                  # the empty slot
    # arg-max positions: the float64 winner, unless its margin is within the fp32 error of a score
    s64, G = r64[1].detach(), slot_idx.shape[0]
    for slot in range(1, G):
        own = torch.nonzero(cand_slot == slot).flatten()
        best = own[s64[own] >= s64[own].max() - 1e-4 * max(1.0, float(s64.abs().max()))]
        assert int(argmax[slot]) in best.tolist(), slot
        if best.numel() == 1:
            assert int(argmax[slot]) == int(r64[3][slot])
    assert attributed(xl.grad, r32[4].grad, r64[4].grad, "d x")
    assert attributed(wl.grad, r32[5].grad, r64[5].grad, "d w")
    assert float(wl.grad[0, D:].abs().max()) > 1e-3                                       # the slot half, through dscores
    assert float(xl.grad[slot_idx[1]].abs().max()) > 0                                    # and a slot row of d x
    hits = int(sum(int(argmax[s]) == int(correct[s]) for s in range(G)))
    assert metrics.tolist() == [hits, G, 1, 0]                                            # one skipped correct index
    _, _, _, _, totals = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot, ops.build_plan([(cand_slot, cand_slot)], G),
                                              w, correct)
    assert totals[1:6].tolist() == [G, hits, 1, 0, cand_idx.shape[0]]


def test_candidate_tie_goes_to_the_lowest_position_and_bad_nodes_are_counted():
    x = torch.randn(10, 8).to(DEV)
    w = torch.randn(1, 16).to(DEV)
    cand_idx = torch.tensor([4, 7, 4, 4, 12, -3], device=DEV)          # node 4 three times; two ids outside [0, 10)
    cand_slot = torch.tensor([1, 0, 1, 1, 0, 0], device=DEV)
    slot_idx = torch.tensor([2, 3], device=DEV)
    x[4] = 100.0 * w[0, :8].sign()                                     # node 4 wins slot 1 by a wide margin: a three-way tie
    plan = ops.build_plan([(cand_slot, cand_slot)], 2)
    _, scores, lse, argmax, totals = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot, plan, w, None)
    assert int(argmax[1]) == 0 and float(scores[0]) == float(scores[2]) == float(scores[3])
    assert int(totals[4]) == 2                                         # clamped and counted, never used as an index
    assert bool(torch.isfinite(lse).all())


def test_candidate_slots_whose_first_candidate_scores_minus_infinity():
    """The edge rule of csrc/softmax_state.h through soft_push_lowest: the candidate a wave meets first (the first of the
    slot in plan order) scores -inf and is taken unconditionally; finite ones behind it (slot 0: wave 0 also has the
    slot's fifth) forget it, and a wave that holds nothing else (slot 1: three candidates, one per wave) adds nothing
    to the slot's sum.  Slot 2 is finite.  A slot of -inf only cannot be built: its slot's own term is finite."""
    D, slot_sizes = 8, [6, 3, 2]
    gen = torch.Generator().manual_seed(4000)
    G, Cn = len(slot_sizes), sum(slot_sizes)
    cand_slot = torch.repeat_interleave(torch.arange(G), torch.tensor(slot_sizes))[torch.randperm(Cn, generator=gen)]
    cand_idx, slot_idx = torch.arange(Cn), torch.arange(Cn, Cn + G)                       # candidate c is node c
    x, w = torch.randn(Cn + G, D, generator=gen), torch.randn(1, 2 * D, generator=gen)
    w[0, 0] = 0.75                                                                        # -inf * w stays -inf
    plan = ops.build_plan([(cand_slot.to(DEV), cand_slot.to(DEV))], G)
    plan.wait()
    rowptr, perm = plan.rowptr.cpu().tolist(), plan.perm.cpu().tolist()
    firsts = [perm[rowptr[g]] for g in (0, 1)]
    assert [int(cand_slot[c]) for c in firsts] == [0, 1]
    x[firsts, 0] = -INF
    _, scores, lse, argmax, _ = ops.candidate_scores(x.to(DEV), cand_idx.to(DEV), slot_idx.to(DEV), cand_slot.to(DEV), plan,
                                                     w.to(DEV), None)
    want = {}
    for dt in (torch.float32, torch.float64):                                             # on the CPU
        s = x.to(dt)[cand_idx] @ w.to(dt)[0, :D] + (x.to(dt)[slot_idx] @ w.to(dt)[0, D:])[cand_slot]
        want[dt] = s, torch.stack([torch.logsumexp(s[cand_slot == g], dim=0) for g in range(G)])
    s64, lse64 = want[torch.float64]
    assert (s64 == -INF).nonzero().flatten().tolist() == sorted(firsts) and bool(torch.isfinite(lse64).all())
    assert not bool(torch.isnan(scores).any()) and not bool(torch.isnan(lse).any())
    assert attributed(scores, want[torch.float32][0], s64, "scores")                      # -inf at the same positions
    assert attributed(lse, want[torch.float32][1], lse64, "lse")
    for g in range(G):
        own = torch.nonzero(cand_slot == g).flatten()
        top2 = s64[own].topk(2)[0]
        assert float(top2[0] - top2[1]) > 1e-3                                            # a decision fp32 resolves
        assert int(argmax[g]) == int(own[s64[own].argmax()]), g


@pytest.mark.parametrize("D", [64, 6], ids=["kernel", "composed"])
def test_skipped_correct_indices_give_their_slot_neither_loss_nor_gradient(D):
    """Non-empty slots whose correct index is outside [0, Cn) or is a candidate of ANOTHER slot: no term of the loss, counted,
    and no loss gradient for the slot's candidates, its slot node or w -- on the kernel and on the composed route."""
    gen = torch.Generator().manual_seed(4000 + D)
    x, w, cand_idx, slot_idx, cand_slot, correct = candidate_batch(D, gen)
    Cn, G = cand_idx.shape[0], slot_idx.shape[0]
    correct[2] = Cn + 7                                                  # 63 candidates, an index past the end
    correct[4] = int(torch.nonzero(cand_slot == 5).flatten()[11])        # 65 candidates, a candidate of slot 5
    x, w, cand_idx, slot_idx, cand_slot, correct = (t.to(DEV) for t in (x, w, cand_idx, slot_idx, cand_slot, correct))
    g = torch.tensor(1.75, device=DEV)
    if D == 64:
        cot = torch.randn(Cn, generator=gen).to(DEV)
        xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        metrics = ops.head_metrics_block(DEV)
        loss, scores, _, argmax = heads.candidate_loss(xl, wl, cand_idx, slot_idx, cand_slot, correct, metrics)
        (loss * g + (scores * cot).sum()).backward()
        grad_x, grad_w = xl.grad, wl.grad
        _, _, _, _, totals = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot,
                                                  ops.build_plan([(cand_slot, cand_slot)], G), w, correct)
        assert int(totals[3]) == 3                                       # the empty slot's -1 and the two above
        # without an extra gradient of the scores the skipped slots get exact zeros
        xz, wz = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        heads.candidate_loss(xz, wz, cand_idx, slot_idx, cand_slot, correct)[0].backward()
        only2 = cand_idx[cand_slot == 2]
        elsewhere = torch.cat([cand_idx[(cand_slot != 2)], slot_idx[[1, 3, 4, 5]]])
        quiet = only2[~torch.isin(only2, elsewhere)]
        assert quiet.numel() > 0 and not bool(xz.grad[quiet].any())
    else:
        cot = torch.zeros(Cn, device=DEV)
        module = heads.VarMisuseGraphModel(StubGnn(D, GnnOutput)).to(DEV)
        (param,) = list(module.parameters())
        with torch.no_grad():
            param.copy_(w)
        xl = x.clone().requires_grad_(True)
        data = dict(node_states=xl, references={"candidate_nodes": cand_idx, "slot_node_idx": slot_idx},
                    reference_graphs={"candidate_nodes": cand_slot}, num_graphs=G)
        with no_blocking_reads():
            loss = module(data, correct)
            (loss * g).backward()
        grad_x, grad_w = xl.grad, param.grad
        (metrics,) = module._VarMisuseGraphModel__device_metrics.blocks.values()
    r32 = candidate_ref(x, w, cand_idx, slot_idx, cand_slot, correct, cot, g, torch.float32)
    r64 = candidate_ref(x, w, cand_idx, slot_idx, cand_slot, correct, cot, g, torch.float64)
    assert attributed(loss, r32[0], r64[0], "loss")
    assert attributed(grad_x, r32[4].grad, r64[4].grad, "d x")
    assert attributed(grad_w, r32[5].grad, r64[5].grad, "d w")
    assert metrics.tolist()[1:3] == [G, 3]


@pytest.mark.parametrize("H", [6, 1028])
def test_widths_beyond_the_candidate_kernel_take_the_composed_route(H):
    gen = torch.Generator().manual_seed(3000 + H)
    sizes = [1, 4, 2, 9, 3]
    G, Cn, N = len(sizes), sum(sizes), 40
    cand_slot = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))[torch.randperm(Cn, generator=gen)]
    cand_idx, slot_idx = torch.randperm(N, generator=gen)[:Cn], torch.randint(0, N, (G,), generator=gen)
    correct = torch.tensor([int(torch.nonzero(cand_slot == s).flatten()[0]) for s in range(G)])
    x = torch.randn(N, H, generator=gen)
    module = heads.VarMisuseGraphModel(StubGnn(H, GnnOutput)).to(DEV)
    w = module.state_dict()["_VarMisuseGraphModel__candidate_scores.weight"]
    inputs = dict(node_states=x, candidate_nodes=cand_idx, candidate_slots=cand_slot, slot_nodes=slot_idx, targets=correct)
    states = x.to(DEV).requires_grad_(True)
    before = ops.launch_counts(aggregation=True, heads=True)
    with no_vendor_calls(), no_blocking_reads():
        loss = module(*call_args("vm", inputs, to=to_dev, states=states))
        loss.backward()
    ran = ops.launches_since(before)
    assert "candidate_scores" not in ran and "candidate_scores_backward" not in ran, ran
    assert ran.get("k_gather_reduce", 0) >= 1                          # the facade's HIP segment reduces
    dev = [t.to(DEV) for t in (cand_idx, slot_idx, cand_slot, correct)]
    zero, one = torch.zeros(Cn, device=DEV), torch.tensor(1.0, device=DEV)
    r32 = candidate_ref(x.to(DEV), w, *dev, zero, one, torch.float32)
    r64 = candidate_ref(x.to(DEV), w, *dev, zero, one, torch.float64)
    assert attributed(loss, r32[0], r64[0], "loss")
    assert attributed(states.grad, r32[4].grad, r64[4].grad, "d x")
    (grad_w,) = [p.grad for p in module.parameters()]
    assert attributed(grad_w, r32[5].grad, r64[5].grad, "d w")
    hits = int((r64[3] == dev[3]).sum())
    assert module.report_metrics() == {"Accuracy": hits / G}


# ---------------------------------------------------------------------------------------------------------------------
# 6. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    gen = torch.Generator().manual_seed(7)
    logits = ((torch.rand(300, 121, generator=gen) - 0.5) * 50).to(DEV)
    targets = torch.randint(0, 121, (300,), generator=gen).to(DEV)
    bits = (torch.rand(300, 121, generator=gen) < 0.3).to(DEV)
    x, w, cand_idx, slot_idx, cand_slot, correct = (t.to(DEV) for t in candidate_batch(128, gen))

    def run():
        out = []
        for mode, t in (("softmax", targets), ("sigmoid", bits)):
            live = logits.clone().requires_grad_(True)
            loss = heads.logit_loss(live, t, mode)
            loss.backward()
            out += [loss.detach(), live.grad]
        xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        loss, scores, lse, argmax = heads.candidate_loss(xl, wl, cand_idx, slot_idx, cand_slot, correct)
        (loss + scores.sum()).backward()
        return out + [loss.detach(), scores.detach(), lse, argmax, xl.grad, wl.grad]

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


def test_a_slot_has_the_same_bits_alone_and_inside_a_batch():
    gen = torch.Generator().manual_seed(8)
    x, w, cand_idx, slot_idx, cand_slot, _ = (t.to(DEV) for t in candidate_batch(64, gen))
    G = slot_idx.shape[0]
    _, scores, lse, argmax, _ = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot,
                                                     ops.build_plan([(cand_slot, cand_slot)], G), w, None)
    for slot in (1, 4, 5):
        own = torch.nonzero(cand_slot == slot).flatten()               # in candidate order, as the stable plan keeps them
        alone_slot = torch.zeros(own.shape[0], dtype=torch.int64, device=DEV)
        _, s1, l1, a1, _ = ops.candidate_scores(x, cand_idx[own], slot_idx[slot:slot + 1], alone_slot,
                                                ops.build_plan([(alone_slot, alone_slot)], 1), w, None)
        assert torch.equal(s1, scores[own]) and torch.equal(l1, lse[slot:slot + 1])
        assert int(own[int(a1[0])]) == int(argmax[slot])


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_the_metrics_block_after_three_calls_is_the_sum_of_three_one_call_blocks(mode):
    gen = torch.Generator().manual_seed(9)
    shared, singles = ops.head_metrics_block(DEV), []
    for R in (50, 129, 7):
        logits = torch.randn(R, 33, generator=gen).to(DEV)
        targets = (torch.randint(0, 33, (R,), generator=gen) if mode == "softmax"
                   else torch.rand(R, 33, generator=gen) < 0.5).to(DEV)
        single = ops.head_metrics_block(DEV)
        ops.logit_loss(logits, targets, mode, shared)
        ops.logit_loss(logits, targets, mode, single)
        singles.append(single.cpu())
    if mode == "softmax":
        assert shared.cpu().tolist() == torch.stack(singles).sum(0).tolist()
    else:
        want = [0.0, 0.0, 0.0]
        for s in singles:                                              # the same float64 additions in the same order
            want = [a + b for a, b in zip(want, s.view(torch.float64)[:3].tolist())]
        assert shared.cpu().view(torch.float64)[:3].tolist() == want
        assert int(shared[3]) == sum(int(s[3]) for s in singles) == 186


# ---------------------------------------------------------------------------------------------------------------------
# 7. AMP dtypes and empty inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kind,name,spec", ALL_HEAD_CASES[1::4], ids=IDS[1::4])
def test_half_node_states_are_upcast_and_the_loss_is_fp32(kind, name, spec, dtype):
    fx, module = fixture_module(kind, name, spec)
    inputs = inputs_of(fx)
    half = inputs["node_states"].to(DEV).to(dtype).requires_grad_(True)
    loss = module(*call_args(kind, inputs, to=to_dev, states=half))
    loss.backward()
    full = half.detach().float().requires_grad_(True)
    want = module(*call_args(kind, inputs, to=to_dev, states=full))
    want.backward()
    assert loss.dtype == torch.float32 and torch.equal(loss, want)     # the same up-cast values: the same bits
    assert half.grad.dtype == dtype and torch.equal(half.grad, full.grad.to(dtype))


def test_no_rows_answer_nan_and_launch_nothing():
    before = ops.launch_counts(heads=True)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    x = torch.randn(6, 8, device=DEV, requires_grad=True)
    g2c = heads.Graph2ClassModule(StubGnn(8, GnnOutput), 5).to(DEV)
    data = dict(node_states=x, references={"supernodes": empty}, reference_graphs={"supernodes": empty}, num_graphs=0)
    loss = g2c(data, empty, None)
    loss.backward()
    probs, classes, graph_idx = g2c.predict(data)
    assert math.isnan(float(loss)) and probs.shape == classes.shape == graph_idx.shape == (0,)
    ppi = heads.PPIClassification(StubGnn(8, GnnOutput), 5).to(DEV)
    none = dict(node_states=torch.zeros(0, 8, device=DEV), references={}, reference_graphs={}, num_graphs=0)
    assert math.isnan(float(ppi(none, torch.zeros(0, 5, dtype=torch.bool, device=DEV))))
    vm = heads.VarMisuseGraphModel(StubGnn(8, GnnOutput)).to(DEV)
    data = dict(node_states=x, references={"candidate_nodes": empty, "slot_node_idx": empty},
                reference_graphs={"candidate_nodes": empty}, num_graphs=0)
    assert math.isnan(float(vm(data, empty)))
    assert ops.launches_since(before) == {}
    for rows in (ops.logit_loss(torch.zeros(0, 5, device=DEV), empty, "softmax"),
                 ops.logit_loss(torch.zeros(0, 5, device=DEV), torch.zeros(0, 5, dtype=torch.bool, device=DEV), "sigmoid")):
        assert math.isnan(float(rows[0])) and rows[4].tolist() == [0] * 8


def test_a_batch_with_an_empty_slot_neither_raises_nor_reads_out_of_range():
    sizes = [3, 0, 2]
    cand_slot = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).to(DEV)
    x = torch.randn(9, 8, device=DEV, requires_grad=True)
    vm = heads.VarMisuseGraphModel(StubGnn(8, GnnOutput)).to(DEV)
    data = dict(node_states=x, references={"candidate_nodes": torch.tensor([0, 1, 2, 3, 4], device=DEV),
                                           "slot_node_idx": torch.tensor([5, 6, 7], device=DEV)},
                reference_graphs={"candidate_nodes": cand_slot}, num_graphs=3)
    loss = vm(data, torch.tensor([1, 5, 3], device=DEV))               # 5 is outside [0, Cn): skipped and counted
    loss.backward()
    assert math.isfinite(float(loss)) and bool(torch.isfinite(x.grad).all())
    assert not bool(x.grad[6].any()) and not bool(x.grad[8].any())     # the empty slot's node and an unused node


# ---------------------------------------------------------------------------------------------------------------------
# 8. LinearFeatureEmbedder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", LFE_CASES, ids=[n for n, _ in LFE_CASES])
def test_linear_feature_embedder_against_its_fixture_on_the_gpu(name, spec):
    fx = load(name)
    module = build_lfe(spec, embeddings)
    module.load_state_dict(state_of(fx), strict=True)
    module = module.to(DEV)
    x = torch.from_numpy(fx["features"]).to(DEV).requires_grad_(True)
    with no_vendor_calls():
        out = module(x)
        (out * torch.from_numpy(fx["cotangent"]).to(DEV)).sum().backward()
    assert close(out, fx["out"]) and close(x.grad, fx["grad.features"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k


@pytest.mark.parametrize("act", [nn.Tanh, nn.ReLU], ids=["tanh", "relu"])
def test_linear_feature_embedder_runs_tanh_and_relu_in_the_gemm_epilogue(act):
    gen = torch.Generator().manual_seed(77)
    torch.manual_seed(77)
    module = embeddings.LinearFeatureEmbedder(48, 64, act())           # widths in fours: the fused node's shape
    x = torch.randn(200, 48, generator=gen)
    cot = torch.randn(200, 64, generator=gen)
    (weight,) = list(module.parameters())

    def reference(dtype):
        xr, wr = x.clone().to(dtype).requires_grad_(True), weight.detach().clone().to(dtype).requires_grad_(True)
        y = xr @ wr.t()
        y = torch.tanh(y) if act is nn.Tanh else torch.relu(y)
        (y * cot.to(dtype)).sum().backward()
        return y, xr.grad, wr.grad

    r32, r64 = reference(torch.float32), reference(torch.float64)
    module = module.to(DEV)
    xl = x.to(DEV).requires_grad_(True)
    before = ops.launch_counts()
    with no_vendor_calls(), mock.patch.object(act, "forward", _refuse(act.__name__ + ".forward")):
        out = module(xl)                                               # the activation module itself never runs
        forward_launches = ops.launches_since(before)
        (out * cot.to(DEV)).sum().backward()
    assert sum(forward_launches.values()) == 1, forward_launches       # one GEMM launch, the activation in its epilogue
    (param,) = list(module.parameters())
    for got, a, b, what in ((out, r32[0], r64[0], "out"), (xl.grad, r32[1], r64[1], "d x"), (param.grad, r32[2], r64[2], "d w")):
        assert attributed(got, a, b, what)
