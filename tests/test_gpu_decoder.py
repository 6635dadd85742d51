"""GruCopyingDecoder on the MI355X: the fused route (csrc/attention_pool.hip with heads := L, csrc/segment_scores.hip)
against the reference fixtures, the segment-scores kernel against a float64 restatement at every width class, vector
count and chunk boundary, determinism, the two copy routes (rows = x / rows = dropout(W_c x)), the composed route beyond
the fused range, AMP dtypes and the greedy-decode shape."""
import contextlib
import math
from unittest import mock

import pytest
import torch
from torch import nn
from torch.utils._python_dispatch import TorchDispatchMode

from agg_paths import TOL, attributed_ok
from decoder_cases import CASES, build, inputs_of, load, make_inputs, ref_logprobs, ref_loss, state_of, weights_of
from ptgnn_amd import ops, sequence
from segment_batches import segment_lse

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXTURE_TOL = 2e-5          # the bar of tests/test_gpu_attention_pool.py, relative to max(1, max |want|)
INF = float("inf")


def close(got, want, tol=FIXTURE_TOL):
    """Finite entries within tol * max(1, max |want|), -inf entries at the same positions."""
    got, want = got.detach().double().cpu(), torch.as_tensor(want).double().cpu()
    if got.shape != want.shape or not torch.equal(got == -INF, want == -INF):
        return False
    finite = torch.isfinite(want)
    if not bool(finite.any()):
        return True
    err, scale = float((got[finite] - want[finite]).abs().max()), max(1.0, float(want[finite].abs().max()))
    print(f"    |got - want| = {err:.3e} (scale {scale:.3e})")
    return err <= tol * scale


def attributed(got, want32, exact, what=""):
    scale = max(1.0, float(exact.detach().abs().max()))
    print(f"    {what}: |got-fp32|={float((got.detach() - want32.detach()).abs().max()):.3e} "
          f"|got-f64|={float((got.detach().double() - exact.detach()).abs().max()):.3e} scale={scale:.3e}")
    return attributed_ok(got, want32, exact, TOL, scale)


def _refuse(name):
    def raiser(*args, **kwargs):
        raise AssertionError(f"{name} was called on the GPU route")
    return raiser


@contextlib.contextmanager
def no_vendor_calls():
    with mock.patch.object(nn.functional, "linear", _refuse("F.linear")), \
            mock.patch.object(nn.GRU, "forward", _refuse("nn.GRU.forward")), \
            mock.patch.object(nn.GRUCell, "forward", _refuse("nn.GRUCell.forward")):
        yield


class _Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else [out]
        self.ops.append((func.overloadpacket.__name__, [(tuple(t.shape), t.numel(), str(t.dtype)) for t in outs
                                                        if isinstance(t, torch.Tensor)]))
        return out


def fixture_module(name, spec, dropout_rate=0.0):
    fx = load(name)
    module = build(spec, sequence, dropout_rate)
    module.load_state_dict(state_of(fx), strict=True)
    return fx, module.to(DEV)


def grads_of(module, inputs):
    out = {"input_memories": inputs["input_memories"].grad, "initial_states": inputs["initial_states"].grad}
    out.update({k: p.grad for k, p in module.named_parameters()})
    return out


def live_inputs(fx):
    inputs = inputs_of(fx, lambda t: t.to(DEV))
    inputs["input_memories"].requires_grad_(True)
    inputs["initial_states"].requires_grad_(True)
    return inputs


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_reference_fixtures_forward_and_gradients_on_the_gpu(name, spec):
    fx, module = fixture_module(name, spec)
    inputs = live_inputs(fx)
    num_inputs, L = inputs["input_memories"].shape[0], spec["T"] - 1
    limit = num_inputs * L * min(spec["H"], spec["Dm"])
    before = ops.launch_counts(aggregation=True)
    with no_vendor_calls(), _Recorder() as rec:
        loss = module(**inputs)
        loss.backward()
        with torch.no_grad():
            outs = module._compute_logprobs(inputs["initial_states"], inputs["input_memories"],
                                            inputs["input_memories_origin_idx"], inputs["target_token_ids"][:, :-1])
    ran = ops.launches_since(before)
    for kernel in ("attention_pool", "attention_pool_backward", "segment_scores", "segment_scores_backward"):
        assert ran.get(kernel, 0) >= 1, ran
    # No [I, L, .] tensor wider than [I, L]: no floating-point tensor of I * L * min(H, Dm) elements or more is produced.
    # Byte scratch of the library calls is not counted, and neither is the memories' own shape [I, Dm] -- the gradient the
    # test asks for has it, and at L = 1 with Dm > H that shape alone is past the bound.  Only there is it exempt.
    memories_shape = tuple(inputs["input_memories"].shape) if num_inputs * spec["Dm"] >= limit else None
    sizes = sorted(((n, op, shape, dt) for op, ts in rec.ops for shape, n, dt in ts
                    if "float" in dt and shape != memories_shape), reverse=True)
    print(f"  {name}: limit {limit} elements, largest tensors produced {sizes[:3]}")
    assert sizes[0][0] < limit, sizes[:3]
    assert not [t for op, ts in rec.ops for t in ts if len(t[0]) == 3 and t[0][:2] == (num_inputs, L)], "an [I, L, .] tensor"
    assert close(loss, fx["loss"])
    for got, key in zip(outs, ("copy_logprobs", "target_logprobs", "gru_state")):
        assert close(got, fx[key]), key
    for k, g in grads_of(module, inputs).items():
        assert close(g, fx["grad." + k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. the kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
def kernel_case(K, Lv, sizes, scale=1.0, shuffled=True):
    """idx over len(sizes) + 1 samples (the last one empty), rows y, vectors v, the two output gradients."""
    g = torch.Generator().manual_seed(7000 + 13 * K + Lv + sum(sizes))
    G = len(sizes) + 1
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffled:
        idx = idx[torch.randperm(idx.shape[0], generator=g)]
    y = torch.randn(idx.shape[0], K, generator=g) * scale
    v = torch.randn(G, Lv, K, generator=g) / (1.0 if scale != 1.0 else math.sqrt(K))
    gs, gl = torch.randn(idx.shape[0], Lv, generator=g), torch.randn(G, Lv, generator=g)
    return [t.to(DEV) for t in (idx, y, v, gs, gl)] + [G]


def run_kernel(idx, y, v, gs, gl, G, sorted_index=False):
    plan = ops.plan_from_sorted_index(idx, G) if sorted_index else ops.plan_for([(idx, idx)], G)
    scores, lse = ops.segment_scores(y, v, plan)
    gy, gv = ops.segment_scores_backward(y, v, plan, scores, lse, gs, gl)
    return scores, lse, gy, gv


def check_kernel_against_float64(K, Lv, sizes, scale=1.0):
    idx, y, v, gs, gl, G = kernel_case(K, Lv, sizes, scale)
    before = ops.launch_counts(aggregation=True)
    scores, lse, gy, gv = run_kernel(idx, y, v, gs, gl, G)
    assert ops.launches_since(before) == {"segment_scores": 1, "segment_scores_backward": 1}
    empty = torch.tensor([s == 0 for s in sizes] + [True], device=DEV)
    assert torch.equal(lse == -INF, empty.unsqueeze(1).expand(G, Lv))        # -inf exactly on the empty samples
    assert float(gv[empty].abs().max()) == 0.0 and bool(torch.isfinite(gy).all()) and bool(torch.isfinite(gv).all())
    res = {}
    for dt in (torch.float32, torch.float64):
        yr, vr = y.detach().to(dt).requires_grad_(True), v.detach().to(dt).requires_grad_(True)
        s = (vr[idx] * yr.unsqueeze(1)).sum(-1)
        l = segment_lse(s, idx, G)
        ((s * gs.to(dt)).sum() + (l[~empty] * gl.to(dt)[~empty]).sum()).backward()
        res[dt] = {"scores": s.detach(), "lse": l.detach()[~empty], "grad_y": yr.grad, "grad_v": vr.grad}
    if scale != 1.0:
        s = res[torch.float64]["scores"]
        spans = [float(s[idx == b].max() - s[idx == b].min()) for b in range(len(sizes)) if sizes[b] > 1]
        assert max(spans) > 100.0                    # exp overflows without the running max
    got = {"scores": scores, "lse": lse[~empty], "grad_y": gy, "grad_v": gv}
    for k, val in got.items():
        assert attributed(val, res[torch.float32][k], res[torch.float64][k], f"K={K} Lv={Lv} n={sum(sizes)} {k}"), k


@pytest.mark.parametrize("Lv", [1, 5, 8])
@pytest.mark.parametrize("K", [4, 6, 64, 128, 1024])
def test_kernel_against_float64(K, Lv):
    check_kernel_against_float64(K, Lv, [300, 1, 0, 57, 129, 4])


@pytest.mark.parametrize("sizes", [[127], [128], [129], [256, 257]], ids=str)
def test_kernel_chunk_boundaries(sizes):
    check_kernel_against_float64(64, 5, sizes)
    check_kernel_against_float64(6, 3, sizes)


def test_kernel_scores_spanning_more_than_100():
    check_kernel_against_float64(64, 8, [400, 2, 0, 90, 250], scale=8.0)


def test_unsupported_shapes_answer_unsupported():
    from ptgnn_amd import _lib
    assert not ops.segment_scores_supported(128, 9) and not ops.segment_scores_supported(1025, 7)
    assert ops.segment_scores_supported(1024, 8) and ops.segment_scores_supported(1, 1)
    for K, Lv in ((16, 9), (1025, 2)):
        idx, y, v, gs, gl, G = kernel_case(K, Lv, [5, 3])
        plan = ops.plan_for([(idx, idx)], G)
        with pytest.raises(_lib.PtgnnAmdError, match=r"code -2"):
            ops.segment_scores(y, v, plan)
        with pytest.raises(_lib.PtgnnAmdError, match=r"code -2"):
            ops.segment_scores_backward(y, v, plan, gs, gl, gs, gl)


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    case = kernel_case(128, 7, [3000, 1, 0, 500, 129])
    for a, b in zip(run_kernel(*case), run_kernel(*case)):
        assert torch.equal(a, b)
    name, spec = CASES[3]
    fx, module = fixture_module(name, spec)
    runs = []
    for _ in range(2):
        module.zero_grad(set_to_none=True)
        inputs = live_inputs(fx)
        loss = module(**inputs)
        loss.backward()
        runs.append([loss.detach().clone()] + [g.clone() for g in grads_of(module, inputs).values()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("K", [64, 100])
def test_a_sample_scores_to_the_same_bits_alone_and_inside_a_batch(K):
    idx, y, v, gs, gl, G = kernel_case(K, 5, [200, 57, 300, 40], shuffled=False)
    rows = torch.nonzero(idx == 2).flatten()
    scores, lse, gy, gv = run_kernel(idx, y, v, gs, gl, G, sorted_index=True)
    alone = run_kernel(torch.zeros_like(rows), y[rows].contiguous(), v[2:3].contiguous(), gs[rows].contiguous(),
                       gl[2:3].contiguous(), 1, sorted_index=True)
    assert torch.equal(lse[2], alone[1][0]) and torch.equal(gv[2], alone[3][0])
    assert torch.equal(scores[rows], alone[0]) and torch.equal(gy[rows], alone[2])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two copy routes
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorded_score_widths():
    widths, real = [], ops.segment_scores

    def spy(y, v, plan):
        widths.append(int(y.shape[1]))
        return real(y, v, plan)
    with mock.patch.object(ops, "segment_scores", spy):
        yield widths


def run_loss(module, fx, seed=None):
    module.zero_grad(set_to_none=True)
    inputs = live_inputs(fx)
    if seed is not None:
        torch.manual_seed(seed)
    loss = module(**inputs)
    loss.backward()
    return [loss.detach().clone()] + [g.clone() for g in grads_of(module, inputs).values()]


def test_inactive_dropout_scores_the_memories_themselves():
    name, spec = CASES[0]
    assert spec["Dm"] != spec["H"]
    for rate, train in ((0.0, True), (0.5, False)):
        fx, module = fixture_module(name, spec, rate)
        module.train(train)
        with recorded_score_widths() as widths:
            run_loss(module, fx)
        assert widths == [spec["Dm"]], (rate, train, widths)          # rows = x: no [I, H] copy projection


def test_active_dropout_scores_the_projected_rows_and_repeats_under_one_seed():
    name, spec = CASES[0]
    fx, module = fixture_module(name, spec, 0.5)
    module.train()
    with recorded_score_widths() as widths, no_vendor_calls():
        first = run_loss(module, fx, seed=5)
    assert widths == [spec["H"]]                                      # rows = dropout(W_c x), vectors = the GRU states
    second = run_loss(module, fx, seed=5)
    for a, b in zip(first, second):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(first[0], run_loss(module, fx, seed=6)[0])


def test_eval_of_a_dropout_module_equals_the_module_without_dropout():
    name, spec = CASES[0]
    fx, plain = fixture_module(name, spec, 0.0)
    _, dropped = fixture_module(name, spec, 0.5)
    for a, b in zip(run_loss(plain.eval(), fx), run_loss(dropped.eval(), fx)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 7. beyond the fused range, AMP, greedy decoding: against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def restated(module, inputs, fn):
    """{dtype: result of fn(weights, inputs in dtype)} for float32 and float64 on the device."""
    out = {}
    for dt in (torch.float32, torch.float64):
        w = weights_of(module, dt)
        cast = {k: (v.detach().to(dt).requires_grad_(True) if v.is_floating_point() else v) for k, v in inputs.items()}
        out[dt] = fn(w, cast)
    return out


def test_nine_steps_take_the_composed_route():
    spec = dict(CASES[0][1], T=10)
    torch.manual_seed(31)
    module = build(spec, sequence).to(DEV)
    inputs = {k: v.to(DEV) for k, v in make_inputs(spec, torch.Generator().manual_seed(32)).items()}
    inputs["input_memories"].requires_grad_(True)
    inputs["initial_states"].requires_grad_(True)
    before = ops.launch_counts(aggregation=True)
    with no_vendor_calls():
        loss = module(**inputs)
        loss.backward()
    ran = ops.launches_since(before)
    assert "segment_scores" not in ran and "attention_pool" not in ran, ran

    def reference(w, cast):
        loss = ref_loss(w, **cast)
        loss.backward()
        grads = {"input_memories": cast["input_memories"].grad, "initial_states": cast["initial_states"].grad}
        grads.update({k: w[k.split("__", 1)[1]].grad for k, _ in module.named_parameters()})
        return loss.detach(), grads
    res = restated(module, inputs, reference)
    assert attributed(loss, res[torch.float32][0], res[torch.float64][0], "loss")
    for k, g in grads_of(module, inputs).items():
        assert attributed(g, res[torch.float32][1][k], res[torch.float64][1][k], k), k


def test_bfloat16_memories_return_bfloat16_logprobs_equal_to_the_fp32_route_cast_down():
    name, spec = CASES[0]
    fx, module = fixture_module(name, spec)
    inp = inputs_of(fx, lambda t: t.to(DEV))
    x16 = inp["input_memories"].bfloat16()
    args = (inp["input_memories_origin_idx"], inp["target_token_ids"][:, :-1])
    with torch.no_grad():
        copy16, target16, state16 = module._compute_logprobs(inp["initial_states"], x16, *args)
        copy32, target32, state32 = module._compute_logprobs(inp["initial_states"], x16.float(), *args)
    assert copy16.dtype == torch.bfloat16 and target16.dtype == torch.bfloat16
    assert torch.equal(copy16, copy32.bfloat16()) and torch.equal(target16, target32.bfloat16())
    assert torch.equal(state16, state32)


def test_three_greedy_decode_steps_feed_the_state_forward():
    name, spec = CASES[2]
    fx, module = fixture_module(name, spec)
    module.eval()
    inp = inputs_of(fx, lambda t: t.to(DEV))
    x, idx = inp["input_memories"], inp["input_memories_origin_idx"]
    tokens = torch.randint(2, spec["V"], (3, spec["B"], 1), generator=torch.Generator().manual_seed(41)).to(DEV)
    state, got = inp["initial_states"], []
    before = ops.launch_counts(aggregation=True)
    with torch.no_grad(), no_vendor_calls():
        for step in range(3):
            copy, target, gru_state = module._compute_logprobs(state, x, idx, tokens[step])
            assert copy.shape == (x.shape[0], 1) and target.shape == (spec["B"], 1, spec["V"])
            assert gru_state.shape == (1, spec["B"], spec["H"])
            state = gru_state.squeeze(0)
            got.append((copy, target, gru_state))
    assert ops.launches_since(before).get("segment_scores") == 3

    def reference(w, cast):
        with torch.no_grad():
            h, out = cast["initial_states"], []
            for step in range(3):
                out.append(ref_logprobs(w, h, cast["input_memories"], idx, tokens[step]))
                h = out[-1][2].squeeze(0)
        return out
    res = restated(module, {"initial_states": inp["initial_states"], "input_memories": x}, reference)
    for step in range(3):
        for k in range(3):
            assert attributed(got[step][k], res[torch.float32][step][k], res[torch.float64][step][k],
                              f"step {step} output {k}")
