"""The copying decoder's fused loss on the MI355X (csrc/vocab_loss.hip): the three entry points against float64
restatements at every vector-width, column-chunk and row-block boundary, their -inf / out-of-range / determinism rules,
GruCopyingDecoder.fused_loss against `forward` and the decoder's reference fixtures, and Graph2SeqModule against its own.

Boundaries of the implementation: 16-byte loads of 4 columns; a forward workgroup takes 2048 columns in two groups of
1024; a backward workgroup takes 1024 columns of 8 rows (the rows of one grad_bias partial)."""
import contextlib
import math
import types
from unittest import mock

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import decoder_cases
import graph2seq_cases
from agg_paths import TOL, attributed_ok
from ptgnn_amd import heads, ops, reduceops, sequence
from ptgnn_amd.gnn import GnnOutput
from test_gpu_decoder import FIXTURE_TOL, close, no_vendor_calls

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
INF = float("inf")
ROW_BLOCK = 8
VOCABS = [1, 3, 4, 5, 23, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
ROWS = [1, 7, ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1]
EXTRA_MODES = ("null", "finite", "neg_inf", "plus50")
GRAD_MODES = ("both", "no_g_norm", "no_g_picked")
NS = types.SimpleNamespace(Graph2SeqModule=heads.Graph2SeqModule, GruCopyingDecoder=sequence.GruCopyingDecoder,
                           MultiheadSelfAttentionVarSizedElementReduce=reduceops.MultiheadSelfAttentionVarSizedElementReduce,
                           SimpleVarSizedElementReduce=reduceops.SimpleVarSizedElementReduce)


SEQ_KERNELS = ("vocab_loss", "vocab_loss_backward", "copy_loss_finish")


def seq_launches(before):
    """Launches of the three kernels of csrc/vocab_loss.hip since `before = ops.launch_counts(sequence=True)`."""
    return {k: v for k, v in ops.launches_since(before).items() if k in SEQ_KERNELS}


def attributed(got, want32, exact, what=""):
    scale = max(1.0, float(exact.detach().abs().max()))
    print(f"    {what}: |got-fp32|={float((got.detach() - want32.detach()).abs().max()):.3e} "
          f"|got-f64|={float((got.detach().double() - exact.detach()).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 1. entries a and b against float64
# ---------------------------------------------------------------------------------------------------------------------
def boundary_targets(V, R, shift):
    """R targets out of: 0, V - 1 and both sides of every 4 / 1024 / 2048 column boundary below V, starting at `shift`."""
    marks = sorted({c for b in (4, 1024, 2048, 3072, 4096) for c in (b - 1, b) if c < V} | {0, V - 1})
    return torch.tensor([marks[(shift + r) % len(marks)] for r in range(R)], dtype=torch.int64, device=DEV)


def vocab_case(V, R, pad, with_bias, extra_mode, scale, shift=0):
    g = torch.Generator().manual_seed(1000 * V + 10 * R + pad + shift)
    storage = (torch.randn(R, V + pad, generator=g) * scale).to(DEV)
    scores = storage[:, :V]                                            # ld = V + pad
    bias = (torch.randn(V, generator=g) * scale).to(DEV) if with_bias else None
    extra = None
    if extra_mode != "null":
        lse = torch.logsumexp(scores.double() + (bias.double() if with_bias else 0.0), dim=-1)
        extra = (lse + torch.randn(R, generator=g).to(DEV).double() * 2.0).float()
        if extra_mode == "neg_inf":
            extra[::3] = -INF
        if extra_mode == "plus50":
            extra[R - 1] = float(lse[R - 1]) + 50.0
    return scores, bias, extra, boundary_targets(V, R, shift), torch.randn(R, generator=g).to(DEV), \
        torch.randn(R, generator=g).to(DEV)


def restate(scores, bias, extra, targets, g_norm, g_picked, dt):
    """float32 / float64 torch restatement of entries a and b."""
    s = scores.detach().to(dt).clone().requires_grad_(True)
    b = bias.detach().to(dt).requires_grad_(True) if bias is not None else None
    e = extra.detach().to(dt).requires_grad_(True) if extra is not None else None
    full = s + b if b is not None else s
    norm = torch.logsumexp(full, dim=-1)
    if e is not None:
        norm = torch.logaddexp(norm, e)
    picked = full.gather(1, targets.unsqueeze(1)).squeeze(1) - norm
    objective = 0.0
    if g_norm is not None:
        objective = objective + (norm * g_norm.to(dt)).sum()
    if g_picked is not None:
        objective = objective + (picked * g_picked.to(dt)).sum()
    objective.backward()
    out = {"norm": norm.detach(), "picked": picked.detach(), "grad_scores": s.grad}
    if b is not None:
        out["grad_bias"] = b.grad
    else:
        out["grad_bias"] = s.grad.sum(0)                               # the column sum, bias or not
    if e is not None:
        out["grad_extra"] = e.grad
    return out


def run_entries(scores, bias, extra, targets, g_norm, g_picked):
    norm, picked, stats = ops.vocab_loss(scores, bias, extra, targets)
    assert torch.equal(stats.sum(-1), norm)
    grad, grad_extra, grad_bias = ops.vocab_loss_backward(scores, bias, extra, targets, stats, g_norm, g_picked)
    out = {"norm": norm, "picked": picked, "grad_scores": grad, "grad_bias": grad_bias}
    if extra is not None:
        out["grad_extra"] = grad_extra
    return out


def check_against_float64(V, R, pad, with_bias, extra_mode, scale, grad_mode, shift=0):
    scores, bias, extra, targets, g_norm, g_picked = vocab_case(V, R, pad, with_bias, extra_mode, scale, shift)
    assert scores.stride(0) == V + pad or R == 1
    if grad_mode == "no_g_norm":
        g_norm = None
    if grad_mode == "no_g_picked":
        g_picked = None
    before = ops.launch_counts(sequence=True)
    got = run_entries(scores, bias, extra, targets, g_norm, g_picked)
    assert ops.launches_since(before) == {"vocab_loss": 1, "vocab_loss_backward": 1}
    what = f"V={V} R={R} ld=V+{pad} bias={with_bias} extra={extra_mode} scale={scale} grads={grad_mode}"
    res = {dt: restate(scores, bias, extra, targets, g_norm, g_picked, dt) for dt in (torch.float32, torch.float64)}
    if scale != 1.0 and V >= 23:
        full = scores.double() + (bias.double() if with_bias else 0.0)
        assert float((full.max(-1)[0] - full.min(-1)[0]).max()) > 100.0          # exp overflows without the running max
    assert sorted(got) == sorted(res[torch.float64])
    for k, val in got.items():
        assert bool(torch.isfinite(val).all()), (what, k)
        assert attributed(val, res[torch.float32][k], res[torch.float64][k], f"{what} {k}"), (what, k)
    if extra_mode == "neg_inf":                                        # the vocabulary log-sum-exp bit for bit, exact zeros
        rows = extra == -INF
        plain = ops.vocab_loss(scores, bias, None, targets)[0]
        assert torch.equal(got["norm"][rows], plain[rows])
        assert float(got["grad_extra"][rows].abs().max()) == 0.0
    if extra_mode == "plus50":
        assert abs(float(got["norm"][R - 1] - extra[R - 1])) < 1e-4    # the copy term carries the normaliser


@pytest.mark.parametrize("V", VOCABS)
def test_vocab_loss_and_backward_against_float64(V):
    run = 0
    for R in ROWS:
        for pad in (0, 3):
            for with_bias in (True, False):
                for extra_mode in EXTRA_MODES:
                    check_against_float64(V, R, pad, with_bias, extra_mode, (1.0, 60.0)[(run // 3) % 2],
                                          GRAD_MODES[run % 3], shift=run)
                    run += 1


@pytest.mark.parametrize("pad,with_bias,extra_mode,scale,grad_mode", [
    (0, True, "neg_inf", 1.0, "both"), (3, False, "plus50", 60.0, "both"), (0, True, "finite", 60.0, "no_g_norm"),
    (3, True, "null", 1.0, "no_g_picked")])
def test_the_reference_vocabulary_of_20000_columns(pad, with_bias, extra_mode, scale, grad_mode):
    check_against_float64(20000, 14, pad, with_bias, extra_mode, scale, grad_mode)


def test_an_out_of_range_target_gives_a_nan_for_its_row_only():
    for V, R, pad in ((23, 9, 3), (2049, 7, 0)):
        scores, bias, extra, targets, g_norm, g_picked = vocab_case(V, R, pad, True, "finite", 1.0)
        good = run_entries(scores, bias, extra, targets, g_norm, g_picked)
        for bad_value in (V, -1, 2 ** 40):
            bad_targets = targets.clone()
            bad_targets[2 % R] = bad_value
            bad = run_entries(scores, bias, extra, bad_targets, g_norm, g_picked)
            keep = torch.ones(R, dtype=torch.bool, device=DEV)
            keep[2 % R] = False
            assert bool(torch.isnan(bad["picked"][2 % R])) and bool(torch.isfinite(bad["picked"][keep]).all())
            assert torch.equal(bad["picked"][keep], good["picked"][keep]) and torch.equal(bad["norm"], good["norm"])
            assert torch.equal(bad["grad_scores"][keep], good["grad_scores"][keep])
            assert bool(torch.isfinite(bad["grad_scores"]).all())     # the bad row has no picked entry: softmax term only


def test_rows_that_are_or_start_with_minus_infinity():
    """The edge rule of csrc/softmax_state.h for the plain (max, sum) state: a row of -inf stays empty, (-inf, 0), and
    its norm is -inf, never nan; a leading -inf is forgotten by what follows.  9 columns: rows on a 16-byte stride run
    the float4 path over columns 0 .. 7 and the ragged tail for column 8, the others the dword path."""
    rows = torch.tensor([[-INF] * 9, [-INF, 0.5, -1.25, 2.0, 0.25, -0.75, 1.5, -2.0, 1.0]])
    exact = torch.logsumexp(rows.double(), dim=-1)                     # on the CPU
    want32 = torch.logsumexp(rows, dim=-1)
    assert float(exact[0]) == -INF and math.isfinite(float(exact[1]))
    norms = []
    for pad in (3, 0):
        storage = torch.zeros(2, 9 + pad)
        storage[:, :9] = rows
        norm, _, stats = ops.vocab_loss(storage.to(DEV)[:, :9])
        norm = norm.cpu()
        assert torch.equal(norm == -INF, exact == -INF) and torch.equal(torch.isnan(norm), torch.isnan(exact)), pad
        assert stats[0].tolist() == [-INF, 0.0]                        # the empty state, and no logf(0)
        assert attributed(norm[1:], want32[1:], exact[1:], f"norm ld=9+{pad}"), pad
        norms.append(norm)
    assert torch.equal(norms[0], norms[1])                             # the bits do not depend on the load path


def test_two_calls_give_the_same_bits():
    for V, R, pad in ((20000, 14, 0), (2049, 9, 3), (23, 8, 3)):
        case = vocab_case(V, R, pad, True, "neg_inf", 60.0)
        first, second = run_entries(*case), run_entries(*case)
        for k in first:
            assert torch.equal(first[k], second[k]), (V, k)
        # the bits do not depend on the alignment of the rows either: thread t owns the same columns on both load paths
        aligned = run_entries(case[0].contiguous() if pad else case[0], *case[1:])
        for k in first:
            assert torch.equal(first[k], aligned[k]), (V, k)


def test_no_rows_launch_nothing():
    before = ops.launch_counts(sequence=True)
    scores = torch.zeros(0, 23, device=DEV)
    norm, picked, stats = ops.vocab_loss(scores, None, None, torch.zeros(0, dtype=torch.int64, device=DEV))
    grad, grad_extra, grad_bias = ops.vocab_loss_backward(scores, None, None, None, stats, None, None)
    assert norm.shape == (0,) and picked.shape == (0,) and grad.shape == (0, 23) and grad_extra is None
    assert float(grad_bias.abs().max()) == 0.0 and ops.launches_since(before) == {}


# ---------------------------------------------------------------------------------------------------------------------
# 2. entry c against float64
# ---------------------------------------------------------------------------------------------------------------------
UNK = 1


def finish_case(B, L):
    g = torch.Generator().manual_seed(500 + 10 * B + L)
    gen = (torch.randn(B, L, generator=g) * 3.0 - 5.0).to(DEV)
    counts = (torch.rand(B * L, generator=g) < 0.4).long() * torch.randint(1, 4, (B * L,), generator=g)
    counts[0] = 2                                                      # location (0, 0): UNK with a copy
    rowptr = torch.cat((torch.zeros(1, dtype=torch.int64), counts.cumsum(0))).to(torch.int32).to(DEV)
    has_copy = (counts > 0).reshape(B, L).to(DEV)
    copied = torch.where(has_copy, (torch.randn(B, L, generator=g) * 3.0 - 4.0).to(DEV), torch.tensor(-INF, device=DEV))
    targets = torch.randint(0, 4, (B, L), generator=g)
    targets[0, 0] = UNK
    lengths = torch.tensor([1 + (b % L) for b in range(B)], dtype=torch.int64)                 # 1 ... L
    return gen, copied, rowptr, has_copy, targets.to(DEV), lengths.to(DEV)


def finish_restated(gen, copied, has_copy, targets, lengths, dt):
    g, c = (t.detach().to(dt).clone().requires_grad_(True) for t in (gen, copied))
    masked = g.masked_fill(has_copy & (targets == UNK), -INF)
    any_correct = torch.logsumexp(torch.stack((masked, c)), dim=0)
    mask = (torch.arange(gen.shape[1], device=DEV).unsqueeze(0) < lengths.unsqueeze(1)).to(dt)
    loss = -((any_correct * mask).sum(-1) / mask.sum(-1)).mean()
    loss.backward()
    return {"loss": loss.detach(), "d_gen": g.grad, "d_copied": c.grad}


@pytest.mark.parametrize("B,L", [(1, 1), (4, 5), (5, 7), (300, 7)])
def test_copy_loss_finish_against_float64(B, L):
    gen, copied, rowptr, has_copy, targets, lengths = finish_case(B, L)
    before = ops.launch_counts(sequence=True)
    loss, d_gen, d_copied = ops.copy_loss_finish(gen, copied, rowptr, targets, UNK, lengths)
    again = ops.copy_loss_finish(gen, copied, rowptr, targets, UNK, lengths)
    assert ops.launches_since(before) == {"copy_loss_finish": 2}
    got = {"loss": loss, "d_gen": d_gen, "d_copied": d_copied}
    for a, b in zip(got.values(), again):
        assert torch.equal(a, b)
    res = {dt: finish_restated(gen, copied, has_copy, targets, lengths, dt) for dt in (torch.float32, torch.float64)}
    for k, val in got.items():
        assert bool(torch.isfinite(val).all()), k
        assert attributed(val, res[torch.float32][k], res[torch.float64][k], f"B={B} L={L} {k}"), k
    unk_with_copy = has_copy & (targets == UNK)
    beyond = torch.arange(L, device=DEV).unsqueeze(0) >= lengths.unsqueeze(1)
    assert bool(unk_with_copy[0, 0]) and (B * L < 20 or bool((unk_with_copy & ~beyond).sum() >= 1))
    assert float(d_gen[unk_with_copy | beyond].abs().sum()) == 0.0                              # exact zeros where masked
    assert float(d_copied[~has_copy | beyond].abs().sum()) == 0.0
    live = ~beyond & ~unk_with_copy
    assert bool((d_gen[live] != 0).all())
    none = ops.copy_loss_finish(gen, copied, None, targets, UNK, lengths)                       # no plan: nothing masked
    want = finish_restated(gen, copied, torch.zeros_like(has_copy), targets, lengths, torch.float64)
    assert close(none[0], want["loss"], 1e-5) and close(none[1], want["d_gen"], 1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fused_loss against forward and the decoder's reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
class _StorageRecorder(TorchDispatchMode):
    """(shape, elements, dtype, storage address) of every tensor an operator returns."""

    def __init__(self):
        super().__init__()
        self.tensors = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in (out if isinstance(out, (tuple, list)) else [out]):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                self.tensors.append((tuple(t.shape), t.numel(), str(t.dtype), t.untyped_storage().data_ptr()))
        return out


def decoder_module(name, spec, dropout_rate=0.0):
    fx = decoder_cases.load(name)
    module = decoder_cases.build(spec, sequence, dropout_rate)
    module.load_state_dict(decoder_cases.state_of(fx), strict=True)
    return fx, module.to(DEV)


def live_inputs(fx):
    inputs = decoder_cases.inputs_of(fx, lambda t: t.to(DEV))
    inputs["input_memories"].requires_grad_(True)
    inputs["initial_states"].requires_grad_(True)
    return inputs


def grads_of(module, inputs):
    out = {"input_memories": inputs["input_memories"].grad, "initial_states": inputs["initial_states"].grad}
    out.update({k: p.grad for k, p in module.named_parameters()})
    return out


@pytest.mark.parametrize("name,spec", decoder_cases.CASES, ids=[n for n, _ in decoder_cases.CASES])
def test_fused_loss_against_forward_and_the_reference_fixture(name, spec):
    fx, module = decoder_module(name, spec)
    inputs = live_inputs(fx)
    I, L, R, V = inputs["input_memories"].shape[0], spec["T"] - 1, spec["B"] * (spec["T"] - 1), spec["V"]
    before = ops.launch_counts(aggregation=True, sequence=True)
    with no_vendor_calls(), _StorageRecorder() as rec:
        loss = module.fused_loss(**inputs)
        loss.backward()
    ran = ops.launches_since(before)
    assert {k: ran.get(k) for k in ("vocab_loss", "vocab_loss_backward", "copy_loss_finish")} == \
        {"vocab_loss": 1, "vocab_loss_backward": 1, "copy_loss_finish": 1}, ran
    assert ran.get("segment_scores") == 1 and ran.get("attention_pool") == 1, ran
    floats = [t for t in rec.tensors if "float" in t[2]]
    assert R * V not in (I * L, I * spec["Dm"], V * spec["E"])           # the count below is about [R, V] alone
    wide = {t[3] for t in floats if t[1] == R * V}
    assert len(wide) == 2, sorted(t for t in floats if t[1] == R * V)  # the raw scores and their gradient
    assert not [t for t in floats if t[0] in ((spec["B"], L, V), (spec["B"], L, V + 1))]      # no target_logprobs, no cat
    assert len({t[3] for t in floats if t[0] == (I, L)}) <= 2           # the copy scores and their gradient
    assert close(loss, fx["loss"])
    fused = grads_of(module, inputs)
    for k, g in fused.items():
        assert close(g, fx["grad." + k]), k
    module.zero_grad(set_to_none=True)
    plain_inputs = live_inputs(fx)
    plain = module(**plain_inputs)
    plain.backward()
    assert close(loss, plain, 1e-5)
    for k, g in grads_of(module, plain_inputs).items():
        assert close(fused[k], g, FIXTURE_TOL), k


def test_fused_loss_of_a_dropout_module():
    name, spec = decoder_cases.CASES[0]
    fx, module = decoder_module(name, spec, 0.2)
    module.eval()                                                      # dropout inactive, fused_loss still runs
    inputs = live_inputs(fx)
    before = ops.launch_counts(sequence=True)
    loss = module.fused_loss(**inputs)
    loss.backward()
    assert seq_launches(before) == {"vocab_loss": 1, "vocab_loss_backward": 1, "copy_loss_finish": 1}
    res = {}
    for dt in (torch.float32, torch.float64):
        w = decoder_cases.weights_of(module, dt)
        cast = {k: (v.detach().to(dt).requires_grad_(True) if v.is_floating_point() else v) for k, v in inputs.items()}
        want = decoder_cases.ref_loss(w, **cast)
        want.backward()
        grads = {"input_memories": cast["input_memories"].grad, "initial_states": cast["initial_states"].grad}
        grads.update({k: w[k.split("__", 1)[1]].grad for k, _ in module.named_parameters()})
        res[dt] = (want.detach(), grads)
    assert attributed(loss, res[torch.float32][0], res[torch.float64][0], "loss")
    for k, g in grads_of(module, inputs).items():
        assert attributed(g, res[torch.float32][1][k], res[torch.float64][1][k], k), k
    module.train()                                                     # a training step: finite, and the same under one seed
    runs = []
    for seed in (5, 5, 6):
        module.zero_grad(set_to_none=True)
        inputs = live_inputs(fx)
        torch.manual_seed(seed)
        with no_vendor_calls():
            loss = module.fused_loss(**inputs)
            loss.backward()
        runs.append([loss.detach().clone()] + [g.clone() for g in grads_of(module, inputs).values()])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(runs[0][0], runs[2][0])


def test_fused_loss_without_copyable_elements_and_with_entries_filed_elsewhere():
    name, spec = decoder_cases.CASES[0]
    fx, module = decoder_module(name, spec)
    L = spec["T"] - 1
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    moved = decoder_cases.inputs_of(fx, lambda t: t.to(DEV))["copyable_elements_sample_idxs"].clone()
    moved[-1] = (moved[-1] + L) % (spec["B"] * L)                     # an entry filed under another sample's location
    for change in (dict(copyable_elements_idxs=empty, copyable_elements_sample_idxs=empty),
                   dict(copyable_elements_sample_idxs=moved)):
        losses, grads = [], []
        for fn in (module.fused_loss, module.forward):
            module.zero_grad(set_to_none=True)
            inputs = dict(live_inputs(fx), **change)
            loss = fn(**inputs)
            loss.backward()
            losses.append(loss.detach())
            grads.append(grads_of(module, inputs))
        assert bool(torch.isfinite(losses[0])) and close(losses[0], losses[1], 1e-5)
        for k in grads[0]:
            assert close(grads[0][k], grads[1][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 4. Graph2SeqModule
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def no_host_reads():
    """Every way a CUDA tensor's value reaches Python raises."""
    def guard(name):
        real = getattr(torch.Tensor, name)

        def guarded(self, *args, **kwargs):
            if self.is_cuda:
                raise AssertionError(f"Tensor.{name} of a CUDA tensor: a blocking read")
            return real(self, *args, **kwargs)
        return mock.patch.object(torch.Tensor, name, guarded)

    with contextlib.ExitStack() as stack:
        for name in ("cpu", "item", "tolist", "__float__"):
            stack.enter_context(guard(name))
        yield


def graph2seq_module(name, spec):
    fx = graph2seq_cases.load(name)
    module = graph2seq_cases.build(spec, NS, GnnOutput)
    module.load_state_dict(graph2seq_cases.state_of(fx), strict=True)
    return fx, module.to(DEV)


def to_dev(t):
    return t.to(DEV)


@pytest.mark.parametrize("name,spec", graph2seq_cases.CASES, ids=[n for n, _ in graph2seq_cases.CASES])
def test_graph2seq_module_against_the_reference_fixture(name, spec):
    fx, module = graph2seq_module(name, spec)
    assert heads.Graph2SeqModule.use_fused_loss is True
    inputs = graph2seq_cases.inputs_of(fx)
    module.reset_metrics()
    states = tuple(inputs[k].to(DEV).requires_grad_(True) for k in ("input_states", "output_states"))
    before = ops.launch_counts(sequence=True)
    with no_vendor_calls(), no_host_reads():
        loss = module(**graph2seq_cases.call_args(spec, inputs, to=to_dev, states=states))
        loss.backward()
        with torch.no_grad():
            second = module(**graph2seq_cases.call_args(spec, inputs, second=True, to=to_dev))
    assert seq_launches(before) == {"vocab_loss": 2, "vocab_loss_backward": 1, "copy_loss_finish": 2}
    assert close(loss, fx["loss"]) and close(second, fx["second.loss"])
    assert close(states[0].grad, fx["grad.input_states"]) and close(states[1].grad, fx["grad.output_states"])
    for k, p in module.named_parameters():
        assert close(p.grad, fx["grad." + k]), k
    assert close(torch.tensor(module.report_metrics()["loss"]), fx["metrics2.loss"])
    module.reset_metrics()
    with torch.no_grad(), no_host_reads():
        module(**graph2seq_cases.call_args(spec, inputs, to=to_dev))
    assert close(torch.tensor(module.report_metrics()["loss"]), fx["metrics1.loss"])


def test_graph2seq_switch_and_bfloat16_node_states():
    name, spec = graph2seq_cases.CASES[0]
    fx, module = graph2seq_module(name, spec)
    inputs = graph2seq_cases.inputs_of(fx)
    half = tuple(inputs[k].to(DEV).bfloat16() for k in ("input_states", "output_states"))
    with torch.no_grad():
        low = module(**graph2seq_cases.call_args(spec, inputs, to=to_dev, states=half))
        up = module(**graph2seq_cases.call_args(spec, inputs, to=to_dev, states=tuple(t.float() for t in half)))
        assert low.dtype == torch.float32 and torch.equal(low, up)
        module.use_fused_loss = False                                  # the module attribute: the decoder's own forward
        before = ops.launch_counts(sequence=True)
        plain = module(**graph2seq_cases.call_args(spec, inputs, to=to_dev))
        assert seq_launches(before) == {}
        assert close(plain, fx["loss"])
