"""Cases of the GruCopyingDecoder fixtures: tests/golden/make_golden_decoder.py builds the modules from the reference's
class, tests/test_decoder_cpu.py and tests/test_gpu_decoder.py from ptgnn_amd.sequence; plus the inputs of a case and a
plain-torch restatement of grucopydecoder.py:70-212 in any dtype on any device (the float64 yardstick of the GPU tests).

A case is V (vocabulary), E (embedding), H (GRU state), Dm (memory width), B samples, T tokens per target (L = T - 1
decoding steps) and the memories per sample.  Every case has a shuffled memory -> sample map with a memory-less sample in
the middle (the last sample has memories: the reference's scatter_add without dim_size answers too few rows otherwise),
an UNK target WITH a valid copy at location (0, 0) -- two entries on that one location, generation masked to -inf there --
an UNK target without a copy at location (B - 1, 0), locations with nothing to copy, and target_lengths shorter than L
for some samples wherever L > 1."""
import glob
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNK_ID = 1

CASES = [
    ("decoder_small", dict(V=50, E=12, H=16, Dm=20, B=4, T=6, sizes=[150, 1, 0, 9], seed=21)),
    ("decoder_odd", dict(V=23, E=10, H=6, Dm=7, B=3, T=4, sizes=[130, 0, 5], seed=22)),     # widths not multiples of 4
    ("decoder_l1", dict(V=50, E=12, H=16, Dm=20, B=4, T=2, sizes=[150, 1, 0, 9], seed=23)),  # the greedy-decode shape
    ("decoder_wide", dict(V=300, E=64, H=128, Dm=128, B=5, T=8, sizes=[300, 1, 0, 57, 129], seed=24)),
]
INPUTS = ("input_memories", "input_memories_origin_idx", "initial_states", "target_token_ids", "copyable_elements_idxs",
          "copyable_elements_sample_idxs", "target_lengths")


def build(spec, ns, dropout_rate=0.0):
    """The decoder of `spec` from the namespace `ns` (a module holding GruCopyingDecoder)."""
    return ns.GruCopyingDecoder(vocabulary_size=spec["V"], embedding_size=spec["E"], hidden_size=spec["H"],
                                memories_hidden_dim=spec["Dm"], unk_id=UNK_ID, dropout_rate=dropout_rate)


def make_inputs(spec, gen):
    """The keyword arguments of GruCopyingDecoder.forward for `spec`, drawn from `gen` (CPU tensors)."""
    B, T, sizes = spec["B"], spec["T"], spec["sizes"]
    L = T - 1
    index = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    index = index[torch.randperm(index.shape[0], generator=gen)]
    memories = torch.randn(index.shape[0], spec["Dm"], generator=gen)
    states = torch.randn(B, spec["H"], generator=gen)
    tokens = torch.randint(2, spec["V"], (B, T), generator=gen)            # no UNK by chance
    tokens[0, 1] = UNK_ID                                                   # location (0, 0): UNK, copyable
    tokens[B - 1, 1] = UNK_ID                                               # location (B - 1, 0): UNK, nothing to copy
    of_sample = [torch.nonzero(index == b).flatten().tolist() for b in range(B)]
    elements, locations = [], []

    def copy(b, step, memory):
        elements.append(memory * L + step)
        locations.append(b * L + step)

    copy(0, 0, of_sample[0][0])
    copy(0, 0, of_sample[0][3])                                             # several entries on one location
    for b in range(B - 1):                                                  # the last sample copies nothing
        for step in range(1, L):
            if of_sample[b] and (b + step) % 2 == 0:
                copy(b, step, of_sample[b][(7 * step + b) % len(of_sample[b])])
    lengths = torch.tensor([max(1, L - (b % 3)) for b in range(B)])
    return dict(input_memories=memories, input_memories_origin_idx=index, initial_states=states,
                target_token_ids=tokens, copyable_elements_idxs=torch.tensor(elements, dtype=torch.int64),
                copyable_elements_sample_idxs=torch.tensor(locations, dtype=torch.int64), target_lengths=lengths)


def files(name):
    return [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".p*.npz")))


def load(name):
    """A fixture (and its continuation files name.pK.npz) as one dict of arrays."""
    out = {}
    for path in files(name):
        z = np.load(path)
        out.update({k: z[k] for k in z.files})
    return out


def state_of(fx):
    return {k[len("state."):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("state.")}


def inputs_of(fx, to=lambda t: t):
    return {k: to(torch.from_numpy(fx[k])) for k in INPUTS}


# ---------------------------------------------------------------------------------------------------------------------
# restatement of grucopydecoder.py:70-212 on plain torch operators (index_add / scatter_reduce instead of torch_scatter,
# an explicit GRU recurrence), dropout 0; `w` maps the reference's parameter names without their class prefix to tensors
# ---------------------------------------------------------------------------------------------------------------------
def weights_of(module, dtype, device=None):
    return {k.split("__", 1)[1]: v.detach().to(device=device or v.device, dtype=dtype).clone().requires_grad_(True)
            for k, v in module.state_dict().items()}


def _segment_lse(scores, index, n):
    top = torch.full((n, scores.shape[1]), -math.inf, dtype=scores.dtype, device=scores.device).scatter_reduce(
        0, index.unsqueeze(1).expand_as(scores), scores.detach(), "amax")
    safe = torch.where(top == -math.inf, torch.zeros_like(top), top)
    total = torch.zeros_like(top).index_add(0, index, (scores - safe[index]).exp())
    return torch.where(top == -math.inf, top, total.log() + safe)


def ref_logprobs(w, initial_states, memories, index, token_ids):
    B, L = token_ids.shape
    H = initial_states.shape[1]
    emb = w["embedding_layer.weight"][token_ids]                                          # [B, L, E]
    h, states = initial_states, []
    for step in range(L):
        gi = emb[:, step] @ w["output_gru.weight_ih_l0"].t() + w["output_gru.bias_ih_l0"]
        gh = h @ w["output_gru.weight_hh_l0"].t() + w["output_gru.bias_hh_l0"]
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        states.append(h)
    o = torch.stack(states, dim=1)                                                         # [B, L, H]
    standard = memories @ w["memories_to_standard_attention.weight"].t()                   # [I, H]
    copy = memories @ w["memories_to_copy_attention.weight"].t()
    per_input = o[index]                                                                   # [I, L, H]
    standard_scores = (per_input * standard.unsqueeze(1)).sum(-1)
    copy_scores = (per_input * copy.unsqueeze(1)).sum(-1)
    probs = (standard_scores - _segment_lse(standard_scores, index, B)[index]).exp()       # [I, L]
    attention = torch.zeros(B, L, H, dtype=o.dtype, device=o.device).index_add(
        0, index, probs.unsqueeze(-1) * standard.unsqueeze(1))
    target_scores = (torch.cat((attention, o), dim=-1) @ w["hidden_to_vocab"]) @ w["embedding_layer.weight"].t() \
        + w["vocab_bias"]
    total_copy = _segment_lse(copy_scores, index, B)                                       # [B, L]
    norm = torch.logsumexp(torch.cat((target_scores, total_copy.unsqueeze(-1)), dim=-1), dim=-1)
    return copy_scores - norm[index], target_scores - norm.unsqueeze(-1), h.unsqueeze(0)


def ref_loss(w, *, input_memories, input_memories_origin_idx, initial_states, target_token_ids, copyable_elements_idxs,
             copyable_elements_sample_idxs, target_lengths):
    copy_logprobs, target_logprobs, _ = ref_logprobs(w, initial_states, input_memories, input_memories_origin_idx,
                                                     target_token_ids[:, :-1])
    B, L = target_token_ids.shape[0], target_token_ids.shape[1] - 1
    valid = torch.zeros(B * L, dtype=torch.int64, device=target_token_ids.device).index_add(
        0, copyable_elements_sample_idxs, torch.ones_like(copyable_elements_sample_idxs)).reshape(B, L) > 0
    generation = torch.gather(target_logprobs, -1, target_token_ids[:, 1:].unsqueeze(-1)).squeeze(-1)
    generation = generation.masked_fill(valid & (target_token_ids[:, 1:] == UNK_ID), -math.inf)
    copied = _segment_lse(copy_logprobs.flatten()[copyable_elements_idxs].unsqueeze(1), copyable_elements_sample_idxs,
                          B * L).reshape(B, L)
    any_correct = torch.logsumexp(torch.stack((generation, copied)), dim=0)
    mask = (torch.arange(L, device=target_lengths.device).unsqueeze(0) < target_lengths.unsqueeze(1)).to(any_correct.dtype)
    return -((any_correct * mask).sum(-1) / mask.sum(-1)).mean()
