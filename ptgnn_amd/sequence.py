"""The copying decoder of the Graph2Seq task: mirror of ptgnn/neuralmodels/sequence/grucopydecoder.py:29-212
(`GruCopyingDecoder`: same class name, constructor keywords, submodule / parameter creation order and name-mangled
parameter names, so a reference state_dict loads strictly and the same seed gives the same initial values).
`GruCopyingDecoderModel` -- vocabulary, tensorisation and the Python greedy-decode loop -- works unchanged around it;
`GruCopyingDecoder.greedy_decode` is that loop (grucopydecoder.py:375-457) on device tensors, one HIP launch of
csrc/decode_step.hip per step in place of `target_logprobs`, torch.topk, the three host copies and the dict merge;
`GruCopyingDecoder.beam_decode` extends its dictionary to a beam search, which the reference does not have.

GPU route (L = decoding steps <= 8, memory and state widths <= 1024), with x the memories [I, Dm], g their sample, o the
GRU's output states [B, L, H]:
  * token embeddings by the HIP row gather (backward: the deterministic segment sum over a plan of the token ids), the GRU
    as L calls of the fused cell -- no vendor RNN;
  * standard attention: the memory Linear commutes with the pool, so u = W_s^T o on the samples, the fused attention pool
    with heads := L (csrc/attention_pool.hip), A = W_s P on the samples -- no [I, H] projection, no [I, L, H] product;
  * copy attention: scores and their per-sample log-sum-exp in one pass (csrc/segment_scores.hip).  Dropout sits between
    the copy Linear and the dot product (grucopydecoder.py:83-97), so while it is active the rows are dropout(W_c x) and
    the vectors o; otherwise W_c moves onto the samples too and the rows are x itself (greedy decoding: L = 1 per step);
  * the vocabulary product as two HIP Linears; in `forward` / `_compute_logprobs` the joint normaliser and the loss
    arithmetic are torch glue on [B, L, V] and [I, L] tensors;
  * `greedy_decode` keeps the hidden state, the next tokens, the done flags, the lengths, the log-probabilities and the
    token matrix on the device for all `max_seq_len` steps: per step the GRU cell, the attention pool and the copy scores
    with L = 1, the RAW vocabulary product, and `ops.decode_step`, which reads those scores and the copy scores and writes
    the prediction.  The memories ordered by (sample, value id) -- `ops.value_groups`, two stable plan builds -- and the
    plan of the memory -> sample map are built once per call.  Nothing is read back inside the loop;
  * `beam_decode` is that loop for W <= 8 hypotheses per sample: the GRU cell and the vocabulary product on B W rows, the
    attention pool and the copy scores with L := W (the hypotheses of a sample are its heads), `ops.beam_step`
    (csrc/beam_step.hip), which writes the W best continuations of every sample, their parents and the reordered
    token histories into a second set of state buffers, and the row gather of the new hidden states by parent.  With
    `length_penalty` > 0 or `early_exit` > 0 it takes the finishing route: `ops.beam_step_links` places the candidates
    by length-normalised key, writes a back-pointer pair per slot in place of the history and counts the live slots;
    `ops.beam_backtrack` writes the histories once after the loop; the host leaves the loop on a lagged read-back of the
    live count (`_LiveWatch`), which `greedy_decode(early_exit=n)` shares;
  * `fused_loss` (the training loss, what `heads.Graph2SeqModule` calls) keeps the same GRU, attention and copy scores and
    replaces that glue by csrc/vocab_loss.hip: `_VocabLoss` reads the RAW second Linear's output once -- bias, running
    maximum, joint normaliser with the copy term, the correct tokens' entries -- and its one-pass backward writes the
    gradient of the raw scores and the bias gradient; the correct copy entries are [C]-sized gathers off the copy scores
    minus the normaliser of their own (sample of the memory, step), their per-location log-sum-exp runs on the facade's
    segment kernels, and `_CopyLossFinish` is the [B, L] tail in one launch.  Neither `target_logprobs` [B, L, V] nor
    `copy_logprobs` [I, L] exists on that route; on shapes beyond the fused range only its attention part is composed.
Shapes beyond that range compose the reference's operator sequence from the HIP Linear, the fused cell, the row gather
and the facade's segment kernels.  CPU tensors take the reference's own operator order on torch (device dispatch as in
every layer of the package); fp16 / bf16 inputs are up-cast on entry and the results cast back.
"""
import math

import torch
from torch import nn

from ptgnn_amd import _lib, _readback, dense, ops, scatter as scatter_facade
from ptgnn_amd.layers import _index_plan, _no_grad_needed
from ptgnn_amd.reduceops import _AttentionPool
from ptgnn_amd.scatter import gather_rows as gather_rows_autograd, segment_scores

_HALF = (torch.float16, torch.bfloat16)
_LIVE_IN_FLIGHT = []         # read-backs of live counts that a decode loop left without looking at: reaped by the next call


def _early_exit_lag(who: str, early_exit) -> int:
    if isinstance(early_exit, bool) or not isinstance(early_exit, int) or early_exit < 0:
        raise _lib.PtgnnAmdError(f"{who}: early_exit must be 0 (off) or a lag of n >= 1 steps (got {early_exit!r})")
    return early_exit


class _LiveWatch:
    """The early exit of a device decode loop.  `live` int32 [T], zeroed once, is what the step kernels count the live
    hypotheses of each step into.  After issuing step s the loop asks `nothing_live(s)`: the count of step s is sent on
    its way to the host, and from s >= lag on the host waits for the read-back of step s - lag -- on that read-back's OWN
    event, never on the stream -- and is told whether it was 0.  So the loop issues min(T, s* + lag + 1) steps, whatever
    the timing, and never runs more than `lag` steps ahead of a count it has seen."""

    def __init__(self, T: int, device, lag: int):
        for old in _readback.take_arrived(_LIVE_IN_FLIGHT, keep=64):
            old.values()                                        # back to the pool of pinned buffers
        self.live = torch.zeros(T, dtype=torch.int32, device=device)
        self.steps, self.lag = T, lag
        self.sent = {}

    def nothing_live(self, step: int) -> bool:
        if step + self.lag < self.steps:                        # a count nobody will look at is not sent
            self.sent[step] = _readback.Readback(self.live[step:step + 1])
        if step < self.lag:
            return False
        return self.sent.pop(step - self.lag).values(wait=True)[0] == 0

    def close(self) -> None:
        """After the loop: what was sent and not looked at (an exit leaves up to `lag` of them) is reaped by a later call."""
        with _readback.LOCK:
            _LIVE_IN_FLIGHT.extend(self.sent.values())
        self.sent = {}


_MAX_ELEMENT_ID = 1 << 22    # greedy_decode: the value ids of a call index one plan build (a row pointer of that length)


def _rows(table: torch.Tensor, index: torch.Tensor, plan=None) -> torch.Tensor:
    """table[index] on the HIP row gather; with autograd when something needs a gradient (`plan`: the plan of `index`
    over the table's rows, built here when not given)."""
    table = table.contiguous()
    if _no_grad_needed(table):
        return ops.gather_rows(table, index)
    if plan is None:
        plan = ops.plan_for([(index, index)], table.shape[0])
    return gather_rows_autograd(table, index, plan)


class _VocabLoss(torch.autograd.Function):
    """(norm [R], picked [R]) = ops.vocab_loss(raw scores [R, V], bias, total_copy [R], targets [R]) as one node: the joint
    normaliser of grucopydecoder.py:124-130 and the correct tokens' log-probabilities of :178-181 without the [R, V]
    log-probabilities.  The backward is the kernel's second entry point; its grad_scores flows into dense._Linear."""

    @staticmethod
    def forward(ctx, raw_scores, bias, total_copy, targets):
        norm, picked, stats = ops.vocab_loss(raw_scores, bias, total_copy, targets)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw_scores, bias, total_copy, targets, stats)
        return norm, picked

    @staticmethod
    def backward(ctx, g_norm, g_picked):
        raw_scores, bias, total_copy, targets, stats = ctx.saved_tensors
        grad, g_extra, g_bias = ops.vocab_loss_backward(raw_scores, bias, total_copy, targets, stats, g_norm, g_picked,
                                                        want_bias=bias is not None and ctx.needs_input_grad[1])
        return grad, g_bias, g_extra if ctx.needs_input_grad[2] else None, None


class _CopyLossFinish(torch.autograd.Function):
    """loss = ops.copy_loss_finish(gen [B, L], copied [B, L], ...) as one node (grucopydecoder.py:171-212).  The launch
    writes the derivatives of its own loss; the backward scales them by the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, gen, copied, rowptr, targets, unk_id, lengths):
        loss, d_gen, d_copied = ops.copy_loss_finish(gen, copied, rowptr, targets, unk_id, lengths)
        ctx.save_for_backward(d_gen, d_copied)
        return loss

    @staticmethod
    def backward(ctx, g):
        d_gen, d_copied = ctx.saved_tensors
        return d_gen * g, d_copied * g, None, None, None, None


def _plan_logsumexp(x: torch.Tensor, index: torch.Tensor, plan) -> torch.Tensor:
    """scatter_logsumexp(x [C, 1], index, eps=0) over the given plan of `index` (the facade's own sequence,
    scatter.scatter_logsumexp, without a second plan build): -inf for a segment without elements."""
    with torch.no_grad():
        vals, slot = ops.gather_reduce(x.detach(), plan, 1, "max", return_arg=True, type_bits=0, col=plan.perm)
        top = torch.where(slot >= 0, vals, torch.full_like(vals, -math.inf))
        shift = ops.gather_rows(top, index)
    rec = x - shift
    rec = rec.masked_fill(rec.isnan(), -math.inf)
    return scatter_facade.segment_reduce(rec.exp(), plan, "sum").log() + top


class GruCopyingDecoder(nn.Module):
    def __init__(self, vocabulary_size: int, embedding_size: int, hidden_size: int, memories_hidden_dim: int,
                 unk_id: int, dropout_rate: float):
        super().__init__()
        self.__embedding_layer = nn.Embedding(num_embeddings=vocabulary_size, embedding_dim=embedding_size)
        self.__output_gru = nn.GRU(input_size=embedding_size, hidden_size=hidden_size, num_layers=1, batch_first=True)
        self.__unk_id = unk_id
        self.__memories_to_standard_attention = nn.Linear(in_features=memories_hidden_dim, out_features=hidden_size,
                                                          bias=False)
        self.__memories_to_copy_attention = nn.Linear(in_features=memories_hidden_dim, out_features=hidden_size,
                                                      bias=False)
        self.__hidden_to_vocab = nn.Parameter(0.01 * torch.randn((2 * hidden_size, embedding_size)))
        self.__vocab_bias = nn.Parameter(torch.zeros(vocabulary_size))
        self.__dropout = nn.Dropout(dropout_rate)

    # --------------------------------------------------------------------------------------------------------------
    # CPU tensors: grucopydecoder.py:70-142 in the reference's operator order
    # --------------------------------------------------------------------------------------------------------------
    def __host_logprobs(self, initial_states, input_memories, input_memories_origin_idx, input_token_ids):
        num_samples = initial_states.shape[0]
        target_token_embeddings = self.__dropout(self.__embedding_layer(input_token_ids))
        output_states, output_gru_state = self.__output_gru(target_token_embeddings, initial_states.unsqueeze(0))
        output_states = output_states.contiguous()                                         # [B, L, H]
        standard_attention_reps = self.__memories_to_standard_attention(input_memories)    # [I, H]
        copy_attention_reps = self.__dropout(self.__memories_to_copy_attention(input_memories))
        output_states_per_input = output_states[input_memories_origin_idx]                 # [I, L, H]
        standard_attention_scores = torch.einsum("ilh,ih->il", output_states_per_input, standard_attention_reps)
        copy_attention_scores = torch.einsum("ilh,ih->il", output_states_per_input, copy_attention_reps)
        standard_attention_logprobs = scatter_facade.scatter_log_softmax(
            standard_attention_scores, index=input_memories_origin_idx, dim=0, eps=0, dim_size=num_samples)
        standard_attention_mul = torch.einsum("il,ih->ilh", torch.exp(standard_attention_logprobs),
                                              standard_attention_reps)
        standard_attention_out = scatter_facade.scatter_add(standard_attention_mul, index=input_memories_origin_idx,
                                                            dim=0, dim_size=num_samples)  # [B, L, H]
        target_scores = torch.einsum(
            "blh,hd,vd->blv", torch.cat((self.__dropout(standard_attention_out), output_states), dim=-1),
            self.__hidden_to_vocab, self.__dropout(self.__embedding_layer.weight)) + self.__vocab_bias
        total_copy_scores = scatter_facade.scatter_logsumexp(copy_attention_scores, index=input_memories_origin_idx,
                                                             dim=0, dim_size=num_samples, eps=0)   # [B, L]
        all_scores = torch.cat((target_scores, total_copy_scores.unsqueeze(-1)), dim=-1)
        normalizing_const = torch.logsumexp(all_scores, dim=-1)                            # [B, L]
        target_logprobs = target_scores - normalizing_const.unsqueeze(-1)
        copy_logprobs = copy_attention_scores - normalizing_const[input_memories_origin_idx]
        return copy_logprobs, target_logprobs, output_gru_state

    # --------------------------------------------------------------------------------------------------------------
    # GPU tensors
    # --------------------------------------------------------------------------------------------------------------
    def __gru_states(self, initial_states, input_token_ids):
        """[B, L, H] output states of the GRU over the embedded tokens: the HIP row gather, then L fused cells."""
        gru = self.__output_gru
        B, L = input_token_ids.shape
        step_major = input_token_ids.t().contiguous().reshape(-1)                          # row l * B + b
        embedded = self.__dropout(_rows(self.__embedding_layer.weight, step_major))       # [L * B, E]
        h, states = initial_states.contiguous(), []
        for step in range(L):
            h = dense.gru_cell_weights(embedded[step * B:(step + 1) * B], h, gru.weight_ih_l0, gru.weight_hh_l0,
                                       gru.bias_ih_l0, gru.bias_hh_l0)
            states.append(h)
        return torch.stack(states, dim=1), h

    def __raw_vocabulary_scores(self, attention_out, output_states):
        """grucopydecoder.py:111-118 on [B * L, .] matrices: two HIP Linears, the bias not added."""
        hidden = torch.cat((self.__dropout(attention_out), output_states), dim=-1)         # [B * L, 2 H]
        projected = dense.linear(hidden, self.__hidden_to_vocab.t())                       # [B * L, E]
        return dense.linear(projected, self.__dropout(self.__embedding_layer.weight))

    def __vocabulary_scores(self, attention_out, output_states):
        """grucopydecoder.py:111-119: the raw scores and the bias."""
        return self.__raw_vocabulary_scores(attention_out, output_states) + self.__vocab_bias

    def __composed_attention(self, x, index, plan, output_states):
        """L > 8 or a width > 1024: the reference's operator sequence (grucopydecoder.py:79-124) on the HIP Linear, the
        row gather and the facade's segment kernels."""
        B, L, H = output_states.shape
        standard_reps = dense.linear(x, self.__memories_to_standard_attention.weight)      # [I, H]
        copy_reps = self.__dropout(dense.linear(x, self.__memories_to_copy_attention.weight))
        states_per_input = _rows(output_states.reshape(B, L * H), index, plan).reshape(-1, L, H)
        standard_scores = (states_per_input * standard_reps.unsqueeze(1)).sum(-1)          # [I, L]
        copy_scores = (states_per_input * copy_reps.unsqueeze(1)).sum(-1)
        probs = scatter_facade.scatter_log_softmax(standard_scores, index, dim=0, eps=0.0, dim_size=B).exp()
        attention_out = scatter_facade.scatter_add(probs.unsqueeze(-1) * standard_reps.unsqueeze(1), index, dim=0,
                                                   dim_size=B)                            # [B, L, H]
        total_copy = scatter_facade.scatter_logsumexp(copy_scores, index, dim=0, dim_size=B, eps=0.0)
        return attention_out.reshape(B * L, H), copy_scores, total_copy

    @staticmethod
    def __check_index(x, index):
        if index.dtype != torch.int64 or not index.is_cuda or index.dim() != 1 or index.shape[0] != x.shape[0]:
            raise _lib.PtgnnAmdError("GruCopyingDecoder: input_memories_origin_idx must be a CUDA int64 tensor with one "
                                     "entry per memory")

    def __attend(self, output_states, x, index, plan):
        """The attention / copy part of the GPU routes, for L vectors per sample (the L steps of a target, or the L
        hypotheses of a beam): output states [B, L, H] -> (attention output [B L, H], copy scores [I, L], their per-sample
        log-sum-exp [B, L])."""
        w_s, w_c = self.__memories_to_standard_attention.weight, self.__memories_to_copy_attention.weight
        H, Dm = w_s.shape
        B, L = output_states.shape[:2]
        states = output_states.reshape(B * L, H)
        drop = self.training and self.__dropout.p > 0.0
        if not (ops.attention_pool_supported(Dm, L) and ops.segment_scores_supported(H if drop else Dm, L)):
            return self.__composed_attention(x, index, plan, output_states)
        queries = dense.linear(states, w_s.t()).reshape(B, L, Dm)                          # u_s = W_s^T o
        pooled = _AttentionPool.apply(x, queries, plan)                                    # [B, L, Dm]
        attention_out = dense.linear(pooled.reshape(B * L, Dm), w_s)                       # A = W_s P
        if drop:
            rows = dense.linear_act_dropout(x, w_c, None, None, self.__dropout.p, True)
            if rows is None:
                rows = self.__dropout(dense.linear(x, w_c))
            vectors = output_states
        else:
            rows, vectors = x, dense.linear(states, w_c.t()).reshape(B, L, Dm)             # u_c = W_c^T o
        copy_scores, total_copy = segment_scores(rows, vectors.contiguous(), plan)         # [I, L], [B, L]
        return attention_out, copy_scores, total_copy

    def __device_attention(self, initial_states, x, index, input_token_ids):
        """What the loss and greedy decoding share: (GRU states [B L, H], attention output [B L, H], copy scores [I, L],
        their per-sample log-sum-exp [B, L], the GRU's last state [B, H], the plan of `index` over the samples)."""
        self.__check_index(x, index)
        B, L = input_token_ids.shape
        output_states, last_state = self.__gru_states(initial_states, input_token_ids)     # [B, L, H]
        states = output_states.reshape(B * L, output_states.shape[2])
        x = x.contiguous()
        plan = _index_plan(index, B)
        attention_out, copy_scores, total_copy = self.__attend(output_states, x, index, plan)
        return states, attention_out, copy_scores, total_copy, last_state, plan

    def __device_logprobs(self, initial_states, x, index, input_token_ids):
        B, L = input_token_ids.shape
        states, attention_out, copy_scores, total_copy, last_state, plan = self.__device_attention(
            initial_states, x, index, input_token_ids)
        target_scores = self.__vocabulary_scores(attention_out, states).reshape(B, L, -1)  # [B, L, V]
        # logsumexp(cat(target_scores, total_copy)) without the [B, L, V + 1] copy
        normalizing_const = torch.logaddexp(torch.logsumexp(target_scores, dim=-1), total_copy)
        target_logprobs = target_scores - normalizing_const.unsqueeze(-1)
        copy_logprobs = copy_scores - _rows(normalizing_const, index, plan)
        return copy_logprobs, target_logprobs, last_state.unsqueeze(0)

    def _compute_logprobs(self, initial_states, input_memories, input_memories_origin_idx, input_token_ids):
        """
        :param input_memories: [num-inputs-flattened, D]
        :param input_memories_origin_idx: [num-inputs-flattened]
        :param initial_states: [num-targets, H]
        :param input_token_ids: [num-targets, max-seq-size-1]

        :return: the logprobs for all copying locations [num-inputs-flattened, max-seq-size-1], the logprobs for all
            elements in the vocabulary [num-targets, max-seq-size-1, vocab-size] and the GRU's last state [1, num-targets, H]
        """
        dt = input_memories.dtype
        if dt in _HALF or initial_states.dtype in _HALF:         # AMP: fp32 inside, the caller's dtypes outside
            copy_logprobs, target_logprobs, state = self._compute_logprobs(
                initial_states.float(), input_memories.float(), input_memories_origin_idx, input_token_ids)
            return copy_logprobs.to(dt), target_logprobs.to(dt), state.to(initial_states.dtype)
        if not input_memories.is_cuda:    # device dispatch: CPU tensors take the reference's own operator order
            return self.__host_logprobs(initial_states, input_memories, input_memories_origin_idx, input_token_ids)
        return self.__device_logprobs(initial_states, input_memories, input_memories_origin_idx, input_token_ids)

    def forward(self, *, input_memories, input_memories_origin_idx, initial_states, target_token_ids,
                copyable_elements_idxs, copyable_elements_sample_idxs, target_lengths):
        """
        :param input_memories: [num-inputs-flattened, D]
        :param input_memories_origin_idx: [num-inputs-flattened]
        :param initial_states: [num-targets, H]
        :param target_token_ids: [num-targets, max-seq-size]
        :param target_lengths: [num-targets]
        :param copyable_elements_idxs: [num-copyable-elements]
        :param copyable_elements_sample_idxs: [num-copyable-elements]

        :return: the loss (grucopydecoder.py:166-212; the segment sums are the facade's: HIP kernels on GPU tensors).
        """
        copy_logprobs, target_logprobs, _ = self._compute_logprobs(
            initial_states, input_memories, input_memories_origin_idx, target_token_ids[:, :-1])
        copy_logprobs, target_logprobs = copy_logprobs.float(), target_logprobs.float()
        num_targets, num_steps = target_token_ids.shape[0], target_token_ids.shape[1] - 1

        # UNKs are only predicted if we cannot copy.
        num_valid_copy_actions = scatter_facade.scatter_add(
            torch.ones_like(copyable_elements_sample_idxs), index=copyable_elements_sample_idxs, dim=0,
            dim_size=num_targets * num_steps)
        locations_with_valid_copy_actions = num_valid_copy_actions.reshape(num_targets, num_steps) > 0
        unk_prediction_locations = target_token_ids[:, 1:] == self.__unk_id
        mask = locations_with_valid_copy_actions & unk_prediction_locations

        correct_generation_logprobs = torch.gather(target_logprobs, index=target_token_ids[:, 1:].unsqueeze(-1),
                                                   dim=-1).squeeze(-1)                    # [num-targets, num-steps]
        correct_generation_logprobs = correct_generation_logprobs.masked_fill(mask, -math.inf)

        correct_copy_logprobs = scatter_facade.scatter_logsumexp(
            copy_logprobs.flatten()[copyable_elements_idxs], index=copyable_elements_sample_idxs, dim=0,
            dim_size=num_targets * num_steps, eps=0).view(num_targets, num_steps)

        any_correct_action_logprob = torch.logsumexp(
            torch.stack((correct_generation_logprobs, correct_copy_logprobs)), dim=0)     # [num-targets, num-steps]

        mask = torch.arange(num_steps, device=target_lengths.device).unsqueeze(0) < target_lengths.unsqueeze(1)
        per_seq_loss = (any_correct_action_logprob * mask.float()).sum(dim=-1) / mask.float().sum(dim=-1)
        return -per_seq_loss.mean()

    def fused_loss(self, *, input_memories, input_memories_origin_idx, initial_states, target_token_ids,
                   copyable_elements_idxs, copyable_elements_sample_idxs, target_lengths):
        """The loss of `forward` (same keyword arguments, same value) on the fused vocabulary-loss kernels
        (csrc/vocab_loss.hip): neither `target_logprobs` [B, L, V] nor `copy_logprobs` [I, L] exists.  The GRU states, the
        attention and the copy scores are those of `_compute_logprobs`; the raw vocabulary product goes through
        `_VocabLoss` (bias, joint normaliser with the copy term, the correct tokens' entries), the correct copy entries
        are read off the copy scores as [C] tensors, and `_CopyLossFinish` is the [B, L] tail in one launch.  CPU tensors
        and B = 0 / L = 0 are handed to `forward`."""
        B, L = target_token_ids.shape[0], target_token_ids.shape[1] - 1
        if not input_memories.is_cuda or B == 0 or L <= 0:
            return self.forward(
                input_memories=input_memories, input_memories_origin_idx=input_memories_origin_idx,
                initial_states=initial_states, target_token_ids=target_token_ids,
                copyable_elements_idxs=copyable_elements_idxs,
                copyable_elements_sample_idxs=copyable_elements_sample_idxs, target_lengths=target_lengths)
        if input_memories.dtype in _HALF or initial_states.dtype in _HALF:       # AMP: fp32 inside, an fp32 loss
            input_memories, initial_states = input_memories.float(), initial_states.float()
        index = input_memories_origin_idx
        states, attention_out, copy_scores, total_copy, _, _ = self.__device_attention(
            initial_states, input_memories, index, target_token_ids[:, :-1])
        targets = target_token_ids[:, 1:].contiguous()                                     # [B, L]
        raw_scores = self.__raw_vocabulary_scores(attention_out, states)                   # [B * L, V]: the only one
        norm, picked = _VocabLoss.apply(raw_scores, self.__vocab_bias, total_copy.reshape(B * L), targets.reshape(B * L))
        if copyable_elements_idxs.shape[0] == 0:
            copied, rowptr = torch.full((B, L), -math.inf, dtype=torch.float32, device=norm.device), None
        else:
            # entry e = memory * L + step of the flattened copy scores; its normaliser is that of (sample of the memory,
            # step), whatever location the caller files the entry under
            memory = torch.div(copyable_elements_idxs, L, rounding_mode="floor")
            own_location = index[memory] * L + (copyable_elements_idxs - memory * L)
            correct = _rows(copy_scores.reshape(-1, 1), copyable_elements_idxs) \
                - _rows(norm.reshape(-1, 1), own_location)                                 # [C, 1]
            plan = _index_plan(copyable_elements_sample_idxs, B * L)
            copied = _plan_logsumexp(correct, copyable_elements_sample_idxs, plan).reshape(B, L)
            rowptr = plan.rowptr
        return _CopyLossFinish.apply(picked.reshape(B, L), copied, rowptr, targets, self.__unk_id, target_lengths.long())

    # --------------------------------------------------------------------------------------------------------------
    # greedy decoding (grucopydecoder.py:375-457)
    # --------------------------------------------------------------------------------------------------------------
    def __host_greedy_step(self, copy_logprobs, target_logprobs, index, ids, top_k, end_id, step, state):
        """One step of the reference's dict merge on torch operators, on [B, V] / [I] log-probabilities: the K largest
        vocabulary entries (equal values: the lower id first), every (sample, value id) group of copy log-probabilities
        merged onto its vocabulary entry where that is one of the K and onto -inf elsewhere, the arg-max (the
        vocabulary's top-1 before a group of equal value, of two groups the lower id), the state update."""
        done, lengths, logprobs, tokens, next_tokens = state
        B, V = target_logprobs.shape
        order = torch.sort(target_logprobs, dim=-1, descending=True, stable=True).indices
        in_top = torch.zeros(B, V, dtype=torch.bool, device=order.device).scatter_(1, order[:, :min(top_k, V)], True)
        best_id = order[:, 0]
        best = target_logprobs.gather(1, best_id.unsqueeze(1)).squeeze(1)
        if index.shape[0]:
            span = int(ids.max()) + 1
            keys, group = torch.unique(index * span + ids, return_inverse=True)        # sorted by (sample, id)
            sample, gid = torch.div(keys, span, rounding_mode="floor"), keys % span
            G = keys.shape[0]
            top = torch.full((G,), -math.inf, dtype=copy_logprobs.dtype).scatter_reduce(
                0, group, copy_logprobs, "amax", include_self=True)
            shift = torch.where(top == -math.inf, torch.zeros_like(top), top)
            merged = torch.zeros(G, dtype=copy_logprobs.dtype).index_add(
                0, group, (copy_logprobs - shift[group]).exp()).log() + shift
            column = gid.clamp(max=V - 1)
            vocabulary = torch.where((gid < V) & in_top[sample, column], target_logprobs[sample, column],
                                     torch.full_like(merged, -math.inf))
            merged = torch.logaddexp(vocabulary, merged)
            group_best = torch.full((B,), -math.inf, dtype=merged.dtype).scatter_reduce(
                0, sample, merged, "amax", include_self=True)
            position = torch.where(merged == group_best[sample], torch.arange(G), torch.full((G,), G))
            first = torch.full((B,), G, dtype=torch.int64).scatter_reduce(0, sample, position, "amin", include_self=True)
            copied = group_best > best
            predicted = torch.where(copied, gid[first.clamp(max=G - 1)], best_id)
            value = torch.where(copied, group_best, best)
        else:
            predicted, value = best_id, best
        live = ~done
        ends = predicted == end_id
        logprobs += torch.where(live, value.float(), torch.zeros_like(logprobs))
        append = live & ~ends
        tokens[:, step] = torch.where(append, predicted, tokens[:, step])
        lengths += append.long()
        next_tokens.copy_(torch.where(live, torch.where(predicted < V, predicted, torch.full_like(predicted, self.__unk_id)),
                                      torch.full_like(predicted, end_id)))
        done |= live & ends

    def greedy_decode(self, *, input_memories, input_memories_origin_idx, initial_states, input_element_ids, start_id: int,
                      end_id: int, max_seq_len: int, top_k: int = 100, early_exit: int = 0):
        """The greedy decoding of GruCopyingDecoderModel.greedy_decode (grucopydecoder.py:375-457) without its host loop.

        :param input_memories: [num-inputs-flattened, D]
        :param input_memories_origin_idx: [num-inputs-flattened]
        :param initial_states: [num-targets, H]
        :param input_element_ids: int64 [num-inputs-flattened], standing in for the reference's `input_concrete_values`:
            an id < vocabulary size is the vocabulary id of the memory's string, any other id is the caller's key of a
            string that is not in the vocabulary (equal strings, equal keys; keys below 2 ** 22)
        :param start_id, end_id: the vocabulary ids of START and END
        :param top_k: the vocabulary candidates per step (the reference's 100)
        :param early_exit: 0: every call runs `max_seq_len` steps.  n >= 1: the loop ends once every sample has predicted
            END -- the results are the same bits.  CPU tensors leave right after that step s*; on GPU tensors the step
            kernel counts the samples that are still live into an int32 [max_seq_len] tensor, and after issuing step s >= n
            the host waits for the read-back of step s - n's count (on that read-back's own event, not on the stream) and
            leaves when it is 0: exactly min(max_seq_len, s* + n + 1) steps are issued, the host is never more than n
            steps ahead of what it has looked at

        :return: token_ids int64 [num-targets, max_seq_len] (row b holds the lengths[b] predicted tokens of sample b in the
            extended id space, END not included, then -1), lengths int64 [num-targets], logprobs float32 [num-targets]
            (the sum of the chosen log-probabilities, END's included).

        Exact ties, which the reference leaves to torch.topk and to dict order: of equal vocabulary scores the lower id
        counts as the larger (for the top-1 and at the K-th place), the vocabulary's top-1 goes before a copy group of
        equal value, and of two groups the lower id.  The module is treated as in eval(): dropout must be inactive."""
        x, index, h, ids = input_memories, input_memories_origin_idx, initial_states, input_element_ids
        if self.training and self.__dropout.p > 0.0:
            raise _lib.PtgnnAmdError("greedy_decode: dropout is active (call eval() first)")
        V = self.__vocab_bias.shape[0]
        B, T, I = int(h.shape[0]), int(max_seq_len), int(x.shape[0])
        if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] != I or ids.device != x.device:
            raise _lib.PtgnnAmdError("greedy_decode: input_element_ids must be an int64 tensor with one entry per memory, on "
                                     "the memories' device")
        if top_k < 1 or T < 0 or not (0 <= start_id < V and 0 <= end_id < V):
            raise _lib.PtgnnAmdError(f"greedy_decode: needs top_k >= 1, max_seq_len >= 0 and start_id / end_id inside the "
                                     f"vocabulary of {V} (got {top_k}, {T}, {start_id}, {end_id})")
        lag = _early_exit_lag("greedy_decode", early_exit)
        dev = x.device
        tokens = torch.full((B, T), -1, dtype=torch.int64, device=dev)
        lengths = torch.zeros(B, dtype=torch.int64, device=dev)
        logprobs = torch.zeros(B, dtype=torch.float32, device=dev)
        if B == 0 or T == 0:
            return tokens, lengths, logprobs
        span = 1
        if I:
            low, high = (int(v) for v in torch.aminmax(ids))     # the one read-back of the call, before the loop
            if low < 0 or high >= _MAX_ELEMENT_ID:
                raise _lib.PtgnnAmdError(f"greedy_decode: input_element_ids must lie in [0, {_MAX_ELEMENT_ID}) (got "
                                         f"{low} .. {high})")
            span = high + 1
        next_tokens = torch.full((B,), int(start_id), dtype=torch.int64, device=dev)
        with torch.no_grad():
            x, h = x.float(), h.float()                          # AMP: fp32 inside, as everywhere
            if not x.is_cuda:    # device dispatch: CPU tensors take the same algorithm on torch operators
                done = torch.zeros(B, dtype=torch.bool)
                for step in range(T):
                    copy_logprobs, target_logprobs, state = self._compute_logprobs(h, x, index, next_tokens.unsqueeze(1))
                    h = state.squeeze(0)
                    self.__host_greedy_step(copy_logprobs.squeeze(1), target_logprobs.squeeze(1), index, ids, top_k, end_id,
                                            step, (done, lengths, logprobs, tokens, next_tokens))
                    if lag and bool(done.all()):
                        break
                return tokens, lengths, logprobs
            done = torch.zeros(B, dtype=torch.int32, device=dev)
            groups = ops.value_groups(index, ids, B, span)
            watch = _LiveWatch(T, dev, lag) if lag else None
            for step in range(T):
                states, attention_out, copy_scores, total_copy, h, _ = self.__device_attention(
                    h, x, index, next_tokens.unsqueeze(1))
                raw_scores = self.__raw_vocabulary_scores(attention_out, states)           # [B, V]
                if watch is None:
                    ops.decode_step(raw_scores, self.__vocab_bias, copy_scores, total_copy.reshape(B), groups, top_k,
                                    self.__unk_id, end_id, step, done, lengths, logprobs, tokens, next_tokens)
                    continue
                ops.decode_step(raw_scores, self.__vocab_bias, copy_scores, total_copy.reshape(B), groups, top_k,
                                self.__unk_id, end_id, step, done, lengths, logprobs, tokens, next_tokens, live=watch.live)
                if watch.nothing_live(step):
                    break
            if watch is not None:
                watch.close()
            ops.post_index_check(dev)
        return tokens, lengths, logprobs

    # --------------------------------------------------------------------------------------------------------------
    # beam search: greedy decoding's dictionary, the W best continuations of W hypotheses per sample
    # --------------------------------------------------------------------------------------------------------------
    def __host_beam_step(self, copy_logprobs, target_logprobs, row_of_memory, ids, top_k, W, end_id, step, state,
                         key_scale=None):
        """One beam step on torch operators, on [B W, V] / [W I] log-probabilities (row b W + j: slot j of sample b; the
        memories repeated once per slot, `row_of_memory` their rows): per live row the W best vocabulary entries -- with
        the row's value group merged in where the id has one -- and the row's other groups, merged as in
        `__host_greedy_step`; per finished row itself.  The candidates are sorted by (sample, higher score, lower parent,
        the W best vocabulary ids first, lower id) with stable sorts from the last key to the first, and the first W of
        a sample are its new slots.  With `key_scale` (float32 [T + 1], the finishing route) "higher score" is "higher
        key", key = score * key_scale[lengths of the parent + 1] in float32; the state keeps the raw sums.  Returns (state,
        next tokens [B W], parent rows [B W])."""
        beam, done, lengths, tokens = state
        R, V = target_logprobs.shape
        B = R // W
        K = min(top_k, V)
        order = torch.sort(target_logprobs, dim=-1, descending=True, stable=True).indices
        in_top = torch.zeros(R, V, dtype=torch.bool).scatter_(1, order[:, :K], True)
        best_w = order[:, :W]                                                           # [R, W]
        in_best = torch.zeros(R, V, dtype=torch.bool).scatter_(1, best_w, True)
        entries = target_logprobs.clone()
        rows = torch.arange(R)
        cand_row, cand_id = [rows.repeat_interleave(W)], [best_w.reshape(-1)]
        cand_class, cand_value = [torch.zeros(R * W, dtype=torch.int64)], []
        if row_of_memory.shape[0]:
            span = int(ids.max()) + 1
            keys, group = torch.unique(row_of_memory * span + ids, return_inverse=True)  # sorted by (row, id)
            row, gid = torch.div(keys, span, rounding_mode="floor"), keys % span
            G = keys.shape[0]
            top = torch.full((G,), -math.inf, dtype=copy_logprobs.dtype).scatter_reduce(
                0, group, copy_logprobs, "amax", include_self=True)
            shift = torch.where(top == -math.inf, torch.zeros_like(top), top)
            merged = torch.zeros(G, dtype=copy_logprobs.dtype).index_add(
                0, group, (copy_logprobs - shift[group]).exp()).log() + shift
            column = gid.clamp(max=V - 1)
            vocabulary = torch.where((gid < V) & in_top[row, column], target_logprobs[row, column],
                                     torch.full_like(merged, -math.inf))
            merged = torch.logaddexp(vocabulary, merged)
            replaces = (gid < V) & in_best[row, column]              # the group's entry IS that vocabulary entry
            entries[row[replaces], column[replaces]] = merged[replaces]
            cand_row.append(row[~replaces])
            cand_id.append(gid[~replaces])
            cand_class.append(torch.ones(int((~replaces).sum()), dtype=torch.int64))
            cand_value.append(merged[~replaces])
        cand_value.insert(0, entries.gather(1, best_w).reshape(-1))
        cand_row, cand_id, cand_class = torch.cat(cand_row), torch.cat(cand_id), torch.cat(cand_class)
        cand_value = torch.cat(cand_value).float()
        live = ~done.reshape(-1)
        keep = live[cand_row]
        finished = rows[~live]
        cand_row = torch.cat((cand_row[keep], finished))
        cand_id = torch.cat((cand_id[keep], torch.full_like(finished, -1)))
        cand_class = torch.cat((cand_class[keep], torch.zeros_like(finished)))
        score = beam.reshape(-1)[cand_row] + torch.cat((cand_value[keep], torch.zeros(finished.shape[0])))
        placed_by = score if key_scale is None else score * key_scale[lengths.reshape(-1)[cand_row] + 1]
        perm = torch.sort(cand_id, stable=True).indices
        for key, descending in ((cand_class, False), (cand_row % W, False), (placed_by, True),
                                (torch.div(cand_row, W, rounding_mode="floor"), False)):
            perm = perm[torch.sort(key[perm], descending=descending, stable=True).indices]
        sample = torch.div(cand_row[perm], W, rounding_mode="floor")
        starts = torch.zeros(B + 1, dtype=torch.int64)
        starts[1:] = torch.bincount(sample, minlength=B).cumsum(0)
        chosen = perm[torch.arange(perm.shape[0]) - starts[sample] < W]                  # [B W]: every sample has >= W
        parent, predicted = cand_row[chosen], cand_id[chosen]
        was_done = ~live[parent]
        ends = ~was_done & (predicted == end_id)
        append = ~was_done & ~ends
        new_tokens = tokens.reshape(R, -1)[parent].clone()
        new_tokens[append, step] = predicted[append]
        next_tokens = torch.where(was_done, torch.full_like(predicted, end_id),
                                  torch.where(predicted < V, predicted, torch.full_like(predicted, self.__unk_id)))
        state = (score[chosen].reshape(B, W), (was_done | ends).reshape(B, W),
                 (lengths.reshape(-1)[parent] + append.long()).reshape(B, W), new_tokens.reshape(B, W, -1))
        return state, next_tokens, parent

    def beam_decode(self, *, input_memories, input_memories_origin_idx, initial_states, input_element_ids, start_id: int,
                    end_id: int, max_seq_len: int, beam_width: int, top_k: int = 100, length_penalty: float = 0.0,
                    early_exit: int = 0):
        """Beam search over the dictionary of `greedy_decode` (the reference has none: grucopydecoder.py:406-442 extended to
        the W = beam_width best hypotheses of every sample); tensor arguments and the extended id space as there.

        Each sample keeps W slots; before the first step slot 0 is (START, its initial state, score 0) and the others
        are the same hypothesis at -inf.  At each of the `max_seq_len` steps every live slot takes a GRU step on its next
        token and has the entries `greedy_decode` builds for a sample, from its own scores; entry e is the candidate
        (parent, e, score[parent] + logprob(e)), a finished slot is its own single candidate.  The W candidates of a
        sample that come first by: higher score; lower parent; inside a parent the ids of its W best vocabulary entries
        before its other entries (of equal vocabulary scores the lower id is the larger); lower id -- are the new slots
        0 .. W - 1, in that order.  END finishes a hypothesis (its log-probability included), anything else is appended;
        W = 1 is `greedy_decode`.

        :param length_penalty: alpha >= 0 of the GNMT length normalisation.  A hypothesis with n scored decisions (its
            appended tokens, plus one for END once it has finished) is RANKED by key = logprob_sum * scale[n], scale[n] =
            ((5 + n) / 6) ** -alpha, made once per call in float64 for n = 0 .. max_seq_len and rounded to a float32 table
            that the device and the CPU route both multiply by.  All candidates of a parent have the same n, so only the
            selection ACROSS parents changes: "higher score" above reads "higher key".  The slots keep and return the raw
            sums, in key order: with alpha > 0 `logprobs` need not be descending.  alpha = 0: the table is all ones
        :param early_exit: 0, or the lag n >= 1 of `greedy_decode`'s early exit: the loop ends once no slot of any sample
            is live (every later step would be the identity); min(max_seq_len, s* + n + 1) steps on GPU tensors
        Without either the call runs exactly what it ran before there were these keywords.  With either it takes the
        FINISHING route: the same step (ops.beam_step_links: the same candidates kernel), back-pointer pairs in place of
        the histories copied every step, one backtrack launch after the loop (ops.beam_backtrack).  Its results for
        alpha = 0 are the default route's bit for bit, for every `early_exit`.

        :return: token_ids int64 [num-targets, W, max_seq_len] (-1 after the tokens, END not included), lengths int64
            [num-targets, W], logprobs float32 [num-targets, W], descending per sample (alpha = 0).

        On GPU tensors the W hypotheses of a sample ride through the fused attention pool and the copy-score kernel as
        W heads of one launch, the step between them is csrc/beam_step.hip and the hidden states are reordered by the row
        gather; nothing is read back inside the loop.  beam_width <= min(top_k, vocabulary size), and <= 8 (the head
        limit of the fused pool) on GPU tensors; the CPU route takes any."""
        x, index, h, ids = input_memories, input_memories_origin_idx, initial_states, input_element_ids
        if self.training and self.__dropout.p > 0.0:
            raise _lib.PtgnnAmdError("beam_decode: dropout is active (call eval() first)")
        V = self.__vocab_bias.shape[0]
        B, T, I, W = int(h.shape[0]), int(max_seq_len), int(x.shape[0]), int(beam_width)
        if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] != I or ids.device != x.device:
            raise _lib.PtgnnAmdError("beam_decode: input_element_ids must be an int64 tensor with one entry per memory, on "
                                     "the memories' device")
        if top_k < 1 or T < 0 or not (0 <= start_id < V and 0 <= end_id < V):
            raise _lib.PtgnnAmdError(f"beam_decode: needs top_k >= 1, max_seq_len >= 0 and start_id / end_id inside the "
                                     f"vocabulary of {V} (got {top_k}, {T}, {start_id}, {end_id})")
        if not 1 <= W <= min(top_k, V):
            raise _lib.PtgnnAmdError(f"beam_decode: needs 1 <= beam_width <= min(top_k, vocabulary size) = "
                                     f"{min(top_k, V)}, so that every step has beam_width finite candidates (got {W})")
        if x.is_cuda and W > 8:
            raise _lib.PtgnnAmdError(f"beam_decode: beam_width {W} > 8, the head limit of the fused attention pool that "
                                     f"carries the hypotheses of a sample on the GPU")
        lag = _early_exit_lag("beam_decode", early_exit)
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) \
                or not math.isfinite(length_penalty) or length_penalty < 0:
            raise _lib.PtgnnAmdError(f"beam_decode: length_penalty must be a finite number >= 0 (got {length_penalty!r})")
        if length_penalty != 0 or lag:
            return self.__finishing_beam_decode(x, index, h, ids, int(start_id), int(end_id), T, W, int(top_k),
                                                float(length_penalty), lag)
        dev = x.device
        tokens = torch.full((B, W, T), -1, dtype=torch.int64, device=dev)
        lengths = torch.zeros(B, W, dtype=torch.int64, device=dev)
        beam = torch.full((B, W), -math.inf, dtype=torch.float32, device=dev)
        beam[:, :1] = 0.0
        if B == 0 or T == 0:
            return tokens, lengths, beam
        span = 1
        if I:
            low, high = (int(v) for v in torch.aminmax(ids))     # the one read-back of the call, before the loop
            if low < 0 or high >= _MAX_ELEMENT_ID:
                raise _lib.PtgnnAmdError(f"beam_decode: input_element_ids must lie in [0, {_MAX_ELEMENT_ID}) (got "
                                         f"{low} .. {high})")
            span = high + 1
        next_tokens = torch.full((B * W,), int(start_id), dtype=torch.int64, device=dev)
        with torch.no_grad():
            x, h = x.float(), h.float()                          # AMP: fp32 inside, as everywhere
            h = h.unsqueeze(1).expand(B, W, h.shape[1]).reshape(B * W, -1).contiguous()    # row b W + j
            if not x.is_cuda:    # device dispatch: CPU tensors take the same algorithm on torch operators
                slot = torch.arange(W).repeat_interleave(I)      # the memories once per slot, slot-major
                x_rows, row_of_memory, ids_rows = x.repeat(W, 1), index.repeat(W) * W + slot, ids.repeat(W)
                state = (beam, torch.zeros(B, W, dtype=torch.bool), lengths, tokens)
                for step in range(T):
                    copy_logprobs, target_logprobs, new_h = self._compute_logprobs(h, x_rows, row_of_memory,
                                                                                   next_tokens.unsqueeze(1))
                    state, next_tokens, parent = self.__host_beam_step(
                        copy_logprobs.squeeze(1), target_logprobs.squeeze(1), row_of_memory, ids_rows, top_k, W, end_id,
                        step, state)
                    h = new_h.squeeze(0)[parent]
                return state[3], state[2], state[0]
            self.__check_index(x, index)
            x = x.contiguous()
            gru, H = self.__output_gru, h.shape[1]
            plan = _index_plan(index, B)
            groups = ops.value_groups(index, ids, B, span)
            state = (beam, torch.zeros(B, W, dtype=torch.int32, device=dev), lengths, tokens)
            spare = tuple(torch.empty_like(t) for t in state)
            parent_rows = torch.empty(B * W, dtype=torch.int64, device=dev)
            for step in range(T):
                embedded = _rows(self.__embedding_layer.weight, next_tokens)               # [B W, E]
                new_h = dense.gru_cell_weights(embedded, h, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
                                               gru.bias_hh_l0)
                attention_out, copy_scores, total_copy = self.__attend(new_h.reshape(B, W, H), x, index, plan)
                raw_scores = self.__raw_vocabulary_scores(attention_out, new_h)            # [B W, V]
                ops.beam_step(raw_scores, self.__vocab_bias, copy_scores, total_copy, groups, top_k, self.__unk_id, end_id,
                              step, state, spare, next_tokens, parent_rows)
                state, spare = spare, state
                h = ops.gather_rows(new_h, parent_rows)
            ops.post_index_check(dev)
        return state[3], state[2], state[0]

    def __finishing_beam_decode(self, x, index, h, ids, start_id, end_id, T, W, top_k, alpha, lag):
        """`beam_decode` with a length penalty and / or an early exit (the arguments are checked): candidates placed by
        key, and on GPU tensors back-pointers, the live count and one backtrack in place of the copied histories."""
        B, I, dev = int(h.shape[0]), int(x.shape[0]), x.device
        lengths = torch.zeros(B, W, dtype=torch.int64, device=dev)
        beam = torch.full((B, W), -math.inf, dtype=torch.float32, device=dev)
        beam[:, :1] = 0.0
        if B == 0 or T == 0:
            return torch.full((B, W, T), -1, dtype=torch.int64, device=dev), lengths, beam
        span = 1
        if I:
            low, high = (int(v) for v in torch.aminmax(ids))     # before the loop, as on the default route
            if low < 0 or high >= _MAX_ELEMENT_ID:
                raise _lib.PtgnnAmdError(f"beam_decode: input_element_ids must lie in [0, {_MAX_ELEMENT_ID}) (got "
                                         f"{low} .. {high})")
            span = high + 1
        scale = ((5.0 + torch.arange(T + 1, dtype=torch.float64)) / 6.0).pow(-alpha).float()   # float64, rounded once
        if not bool((scale > 0).all()):
            raise _lib.PtgnnAmdError(f"beam_decode: length_penalty {alpha} over {T} steps leaves float32 (a scale of 0)")
        next_tokens = torch.full((B * W,), start_id, dtype=torch.int64, device=dev)
        with torch.no_grad():
            x, h = x.float(), h.float()                          # AMP: fp32 inside, as everywhere
            h = h.unsqueeze(1).expand(B, W, h.shape[1]).reshape(B * W, -1).contiguous()    # row b W + j
            if not x.is_cuda:    # device dispatch: the default route's CPU loop with the key order and the immediate exit
                slot = torch.arange(W).repeat_interleave(I)
                x_rows, row_of_memory, ids_rows = x.repeat(W, 1), index.repeat(W) * W + slot, ids.repeat(W)
                state = (beam, torch.zeros(B, W, dtype=torch.bool), lengths, torch.full((B, W, T), -1, dtype=torch.int64))
                for step in range(T):
                    copy_logprobs, target_logprobs, new_h = self._compute_logprobs(h, x_rows, row_of_memory,
                                                                                   next_tokens.unsqueeze(1))
                    state, next_tokens, parent = self.__host_beam_step(
                        copy_logprobs.squeeze(1), target_logprobs.squeeze(1), row_of_memory, ids_rows, top_k, W, end_id,
                        step, state, key_scale=scale)
                    if lag and bool(state[1].all()):
                        break
                    h = new_h.squeeze(0)[parent]
                return state[3], state[2], state[0]
            self.__check_index(x, index)
            x = x.contiguous()
            gru, H = self.__output_gru, h.shape[1]
            plan = _index_plan(index, B)
            groups = ops.value_groups(index, ids, B, span)
            scale = scale.to(dev)
            state = (beam, torch.zeros(B, W, dtype=torch.int32, device=dev), lengths)
            spare = tuple(torch.empty_like(t) for t in state)
            parent_rows = torch.empty(B * W, dtype=torch.int64, device=dev)
            links = torch.empty(T, B, W, 2, dtype=torch.int32, device=dev)
            watch = _LiveWatch(T, dev, lag) if lag else None
            steps_run = 0
            for step in range(T):
                embedded = _rows(self.__embedding_layer.weight, next_tokens)               # [B W, E]
                new_h = dense.gru_cell_weights(embedded, h, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
                                               gru.bias_hh_l0)
                attention_out, copy_scores, total_copy = self.__attend(new_h.reshape(B, W, H), x, index, plan)
                raw_scores = self.__raw_vocabulary_scores(attention_out, new_h)            # [B W, V]
                ops.beam_step_links(raw_scores, self.__vocab_bias, copy_scores, total_copy, groups, top_k, self.__unk_id,
                                    end_id, step, scale, state, spare, next_tokens, parent_rows, links,
                                    watch.live if watch is not None else None)
                state, spare = spare, state
                steps_run = step + 1
                if watch is not None and watch.nothing_live(step):
                    break
                h = ops.gather_rows(new_h, parent_rows)
            if watch is not None:
                watch.close()
            tokens = torch.empty(B, W, T, dtype=torch.int64, device=dev)                   # every column is written
            ops.beam_backtrack(links, steps_run, tokens)
            ops.post_index_check(dev)
        return tokens, state[2], state[0]

    def forward_sharded(self, *args, **kwargs):
        """The decoder attends over all memories of a sample: there is no sharded form (as for the attention reducers)."""
        raise _lib.PtgnnAmdError("forward_sharded: cannot combine partial pools of GruCopyingDecoder")
