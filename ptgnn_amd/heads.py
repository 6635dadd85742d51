"""The task heads of the three benchmarked models and of Graph2Seq: the `ModuleWithMetrics` that owns the GNN, turns node
states into a loss and keeps the accuracy figures.  Mirrors of

    Graph2ClassModule     ptgnn/implementations/typilus/graph2class.py:63-102
    VarMisuseGraphModel   ptgnn/implementations/varmisuse/varmisuse.py:41-91
    PPIClassification     ptgnn/implementations/ppi/ppi.py:13-62
    Graph2SeqModule       ptgnn/implementations/graph2seq/graph2seq.py:36-81

with the same class names, constructor keywords, RNG draws in the same order, name-mangled parameter names (a reference
state_dict loads strictly, both ways), forward signatures and metric names.  `gnn` is any module with
`output_node_state_dim` whose call returns a `GnnOutput`: the reference's container and `ptgnn_amd.gnn.GraphNeuralNetwork`
both qualify.

GPU route (node states on the GPU; csrc/task_heads.hip):
  * Graph2Class / PPI: the Linear on `dense.linear`, then ONE autograd node around the logit-loss kernel (loss, arg-max /
    tp, fp, fn, and the gradient of the logits in one pass each).  Graph2Class gathers its supernode rows with the
    differentiable HIP row gather, or the plain one -- no plan build -- when nothing needs a gradient.
  * VarMisuse: ONE autograd node around the candidate kernel (no [Cn, 2H] concatenation, no gathered copies; d x by one
    segment sum over the plan of the candidate and slot ids).  Node states whose width is not a multiple of 4 up to 1024
    compose the HIP row gather, `dense.linear` and the facade's scatter_log_softmax / scatter_max.
  * Graph2Seq: the backbone nodes' states by the differentiable HIP row gather, the summariser of `reduceops`, and the
    decoder's loss on the fused vocabulary-loss kernels (`sequence.GruCopyingDecoder.fused_loss`, csrc/vocab_loss.hip);
    the loss is added into a per-device accumulator tensor, read in `_module_metrics` only.
  * fp16 / bf16 node states and parameters are up-cast; the loss is fp32.
  * NO call of `forward` or `predict` waits for the device.  The metrics live in a lazily allocated per-device block that
    the kernels' merge step adds into; they reach the host in `_module_metrics` / `report_metrics` only, where the
    reference reads too.  A block belongs to one stream at a time.
CPU tensors take the reference's own operator sequence and accumulate their metrics as host numbers, like the reference.

Differences from the reference: INTEGRATION.md section 1.
"""
from typing import Any, Dict, Tuple

import torch
from torch import nn

from ptgnn_amd import dense, ops, scatter, sequence
from ptgnn_amd._lib import PtgnnAmdError
from ptgnn_amd.gnn import GnnOutput, ModuleWithMetrics
from ptgnn_amd.reduceops import ElementsToSummaryRepresentationInput

_NAN = float("nan")


class _LogitLoss(torch.autograd.Function):
    """loss = ops.logit_loss(logits, targets, mode) as one node; the backward is the kernel's second entry point, fed the
    upstream scalar and the live-row count on the device."""

    @staticmethod
    def forward(ctx, logits, targets, mode, metrics):
        loss, lse, _, _, totals = ops.logit_loss(logits, targets, mode, metrics)
        ctx.mode = mode
        ctx.save_for_backward(logits, targets, lse, totals)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, targets, lse, totals = ctx.saved_tensors
        return ops.logit_loss_backward(logits, targets, ctx.mode, lse, totals, g), None, None, None


def _nan_loss(device, *inputs) -> torch.Tensor:
    """What the CPU route answers for no rows / nodes / slots: a nan loss whose backward gives `inputs` (node states,
    parameters) zero gradients, as the mean over nothing does.  Nothing of the library is launched."""
    loss = torch.full((), _NAN, dtype=torch.float32, device=device)
    for t in inputs:
        if t is not None and t.requires_grad:
            loss = loss + t.float().sum() * 0.0
    return loss


def logit_loss(logits: torch.Tensor, targets: torch.Tensor, mode: str, metrics=None) -> torch.Tensor:
    """Differentiable row loss over fp32 CUDA logits [R, C]: "softmax" (int64 targets [R], nn.CrossEntropyLoss with its
    ignore_index) or "sigmoid" (bool targets [R, C], BCE-with-logits summed per row, mean over rows).  `metrics`: a block
    of `ops.head_metrics_block` that receives this call's accuracy / precision-recall figures."""
    if logits.shape[0] == 0:        # what the CPU route answers for no rows; nothing is launched
        return _nan_loss(logits.device, logits)
    return _LogitLoss.apply(logits, targets, mode, metrics)


class _CandidateLoss(torch.autograd.Function):
    """(loss, scores, lse, argmax) = ops.candidate_scores(...) as one node.  The backward takes the gradients of the loss
    AND of the scores (the loss alone gives the slot half a mathematically zero gradient: log-softmax is shift-invariant
    per slot), writes the compact [Cn + G, D] row gradients and turns them into d x with one HIP segment sum."""

    @staticmethod
    def forward(ctx, x, w, cand_idx, slot_idx, cand_slot, plan, correct, metrics):
        loss, scores, lse, argmax, _ = ops.candidate_scores(x, cand_idx, slot_idx, cand_slot, plan, w, correct, metrics)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, w, cand_idx, slot_idx, cand_slot, correct, scores, lse)
        ctx.mark_non_differentiable(lse, argmax)
        return loss, scores, lse, argmax

    @staticmethod
    def backward(ctx, g_loss, g_scores, _g_lse, _g_argmax):
        x, w, cand_idx, slot_idx, cand_slot, correct, scores, lse = ctx.saved_tensors
        if correct is None:
            g_loss = None                     # the loss of a call without `correct` is a constant nan
        row_grad, grad_w = ops.candidate_scores_backward(x, cand_idx, slot_idx, cand_slot, ctx.plan, w, correct, scores,
                                                         lse, g_loss, g_scores)
        d_x = None
        if ctx.needs_input_grad[0]:
            Cn = cand_idx.shape[0]
            rows = torch.empty(Cn + slot_idx.shape[0], dtype=torch.int64, device=x.device)
            rows[:Cn] = cand_idx
            rows[Cn:] = slot_idx
            d_x = ops.segment_reduce(row_grad, ops.build_plan([(rows, rows)], x.shape[0]), "sum")
        return d_x, grad_w.reshape(w.shape) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None


def candidate_loss(x: torch.Tensor, w: torch.Tensor, cand_idx: torch.Tensor, slot_idx: torch.Tensor,
                   cand_slot: torch.Tensor, correct=None, metrics=None, plan=None):
    """Differentiable (loss, scores [Cn], lse [G], argmax [G]) of the VarMisuse candidate scoring over fp32 CUDA node states
    x [N, D] (D a multiple of 4 up to 1024: `ops.candidate_scores_supported`) and w [1, 2 D]; `plan`: the segment plan of
    cand_slot over the slots, built here when not given."""
    if plan is None:
        plan = ops.build_plan([(cand_slot, cand_slot)], int(slot_idx.shape[0]))
    return _CandidateLoss.apply(x, w, cand_idx, slot_idx, cand_slot, plan, correct, metrics)


class _DeviceMetrics:
    """The per-device metrics blocks of one head: allocated on first use, dropped (not zeroed: no launch) on reset."""

    def __init__(self):
        self.blocks = {}

    def block(self, device) -> torch.Tensor:
        b = self.blocks.get(device)
        if b is None:
            b = self.blocks[device] = ops.head_metrics_block(device)
        return b

    def read(self):
        """The blocks on the host (a blocking read: only `_module_metrics` comes here)."""
        return [b.cpu() for b in self.blocks.values()]


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 else t.float()


class Graph2ClassModule(ModuleWithMetrics):
    def __init__(self, gnn: nn.Module, num_target_classes: int):
        super().__init__()
        self.__gnn = gnn
        self.__node_to_class = nn.Linear(in_features=gnn.output_node_state_dim, out_features=num_target_classes)
        nn.init.uniform_(self.__node_to_class.weight)
        nn.init.zeros_(self.__node_to_class.bias)
        self.__loss = nn.CrossEntropyLoss()

    def _reset_module_metrics(self) -> None:
        self.__num_samples = 0
        self.__sum_accuracy = 0
        self.__device_metrics = _DeviceMetrics()

    def _module_metrics(self) -> Dict[str, Any]:
        correct, samples = int(self.__sum_accuracy), int(self.__num_samples)
        for b in self.__device_metrics.read():
            correct, samples = correct + int(b[0]), samples + int(b[1])
        return {"Accuracy": correct / samples}

    def _logits(self, graph_mb_data):
        graph_output: GnnOutput = self.__gnn(**graph_mb_data)
        supernode_idxs = graph_output.reference_nodes_idx["supernodes"]
        supernode_graph_idx = graph_output.reference_nodes_graph_idx["supernodes"]
        states = graph_output.output_node_representations
        if not states.is_cuda:            # device dispatch: CPU tensors take the reference's own operator order
            return self.__node_to_class(states[supernode_idxs]), supernode_graph_idx
        x = _f32(states)
        if supernode_idxs.shape[0] == 0:  # no supernodes: nothing is launched
            return x.new_zeros(0, self.__node_to_class.out_features) + x.sum() * 0.0, supernode_graph_idx
        if torch.is_grad_enabled() and x.requires_grad:
            rows = scatter.gather_rows(x, supernode_idxs, ops.build_plan([(supernode_idxs, supernode_idxs)], x.shape[0]))
        else:
            rows = ops.gather_rows(x, supernode_idxs)                         # no plan build
        return dense.linear(rows, _f32(self.__node_to_class.weight), _f32(self.__node_to_class.bias)), supernode_graph_idx

    def predict(self, graph_mb_data) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        with torch.no_grad():
            logits, supernode_graph_idx = self._logits(graph_mb_data)
            if not logits.is_cuda:
                probs = torch.softmax(logits, dim=-1)
                return torch.max(probs, dim=-1) + (supernode_graph_idx,)
            _, _, argmax, max_prob, _ = ops.logit_loss(logits, None, "softmax")
            return max_prob, argmax, supernode_graph_idx

    def forward(self, graph_mb_data, target_classes, original_supernode_idxs):
        logits, _ = self._logits(graph_mb_data)
        if logits.is_cuda and logits.shape[0] == 0:
            return _nan_loss(logits.device, logits, *self.__node_to_class.parameters())
        if logits.is_cuda:
            return logit_loss(logits, target_classes, "softmax", self.__device_metrics.block(logits.device))
        with torch.no_grad():
            self.__sum_accuracy += (torch.argmax(logits, dim=-1) == target_classes).sum()
            self.__num_samples += target_classes.shape[0]
        return self.__loss(logits, target_classes)


class VarMisuseGraphModel(ModuleWithMetrics):
    def __init__(self, gnn: nn.Module):
        super().__init__()
        self._gnn = gnn
        self.__candidate_scores = nn.Linear(self._gnn.output_node_state_dim + self._gnn.output_node_state_dim, 1,
                                            bias=False)

    def _reset_module_metrics(self) -> None:
        self.__sum_acc = 0
        self.__num_samples = 0
        self.__device_metrics = _DeviceMetrics()

    def _module_metrics(self) -> Dict[str, Any]:
        correct, samples = self.__sum_acc, self.__num_samples
        for b in self.__device_metrics.read():
            correct, samples = correct + int(b[0]), samples + int(b[1])
        return {"Accuracy": correct / samples}

    def __composed(self, x, cand_idx, slot_idx, cand_slot, correct):
        """varmisuse.py:63-91 on the HIP row gather, `dense.linear` and the scatter facade, for widths outside the candidate
        kernel: the Linear over the concatenation is the sum of its two halves."""
        N, H, G = x.shape[0], x.shape[1], slot_idx.shape[0]

        def rows_of(t, index, count):
            return scatter.gather_rows(t, index, ops.build_plan([(index, index)], count))

        candidates = rows_of(x, cand_idx, N)
        slots_per_candidate = rows_of(rows_of(x, slot_idx, N), cand_slot, G)
        w = _f32(self.__candidate_scores.weight)
        scores = (dense.linear(candidates, w[:, :H].contiguous())
                  + dense.linear(slots_per_candidate, w[:, H:].contiguous())).squeeze(-1)
        logprobs = scatter.scatter_log_softmax(scores, cand_slot, dim=0, eps=0, dim_size=G)
        # the kernel's rule for correct indices: one that is not a candidate of its own slot is skipped and counted, and
        # never used as an index
        Cn = cand_idx.shape[0]
        safe = correct.clamp(0, max(Cn - 1, 0))
        if Cn == 0:
            ok = torch.zeros_like(correct, dtype=torch.bool)
            terms = logprobs.new_zeros(G)
        else:
            ok = (correct >= 0) & (correct < Cn) & (cand_slot[safe] == torch.arange(G, device=x.device))
            terms = torch.where(ok, logprobs[safe], torch.zeros_like(logprobs[safe]))
        with torch.no_grad():
            block = self.__device_metrics.block(x.device)
            best = scatter.scatter_max(scores.detach(), cand_slot, dim=0, dim_size=G)[1]
            block[0] += (ok & (best == correct)).sum()
            block[1] += G
            block[2] += (~ok).sum()
        return -terms.sum() / G

    def forward(self, graph_data, correct_candidate_idxs):
        gnn_output: GnnOutput = self._gnn(**graph_data)
        states = gnn_output.output_node_representations
        cand_idx = gnn_output.node_idx_references["candidate_nodes"]
        cand_slot = gnn_output.node_graph_idx_reference["candidate_nodes"]
        slot_idx = gnn_output.node_idx_references["slot_node_idx"]
        if states.is_cuda:
            x = _f32(states)
            if slot_idx.shape[0] == 0:
                return _nan_loss(x.device, states, self.__candidate_scores.weight)
            if not ops.candidate_scores_supported(x.shape[1]):
                return self.__composed(x, cand_idx, slot_idx, cand_slot, correct_candidate_idxs)
            return candidate_loss(x, _f32(self.__candidate_scores.weight), cand_idx, slot_idx, cand_slot,
                                  correct_candidate_idxs, self.__device_metrics.block(x.device))[0]
        # CPU tensors: the reference's own operator order (the scatter facade serves host tensors on plain torch)
        candidate_node_representations = states[cand_idx]
        slot_representations = states[slot_idx]
        slot_representations_per_candidate = slot_representations[cand_slot]
        candidate_scores = self.__candidate_scores(
            torch.cat((candidate_node_representations, slot_representations_per_candidate), dim=-1)).squeeze(-1)
        candidate_nodes_logprobs = scatter.scatter_log_softmax(src=candidate_scores, index=cand_slot, eps=0)
        with torch.no_grad():
            self.__sum_acc += int((scatter.scatter_max(candidate_scores, index=cand_slot)[1]
                                   == correct_candidate_idxs).sum())
            self.__num_samples += int(slot_representations.shape[0])
        return -candidate_nodes_logprobs[correct_candidate_idxs].mean()


class PPIClassification(ModuleWithMetrics):
    def __init__(self, gnn: nn.Module, num_target_classes: int):
        super().__init__()
        self.__gnn = gnn
        self.__output_representation_to_logits = nn.Linear(in_features=gnn.output_node_state_dim,
                                                           out_features=num_target_classes)
        nn.init.xavier_uniform_(self.__output_representation_to_logits.weight)
        nn.init.zeros_(self.__output_representation_to_logits.bias)

    def _reset_module_metrics(self) -> None:
        self.__num_samples = 0
        self.__sum_f1 = 0.0
        self.__sum_pr = 0.0
        self.__sum_re = 0.0
        self.__device_metrics = _DeviceMetrics()

    def _module_metrics(self) -> Dict[str, Any]:
        f1, pr, re, samples = self.__sum_f1, self.__sum_pr, self.__sum_re, self.__num_samples
        for b in self.__device_metrics.read():
            sums = b.view(torch.float64)
            pr, re, f1, samples = pr + float(sums[0]), re + float(sums[1]), f1 + float(sums[2]), samples + int(b[3])
        return {"f1_score": f1 / samples, "pr_score": pr / samples, "re_score": re / samples}

    def forward(self, graph_data, targets):
        gnn_output: GnnOutput = self.__gnn(**graph_data)
        states = gnn_output.output_node_representations
        linear = self.__output_representation_to_logits
        if states.is_cuda:
            if states.shape[0] == 0:
                return _nan_loss(states.device, states, linear.weight, linear.bias)
            target_logits = dense.linear(_f32(states), _f32(linear.weight), _f32(linear.bias))
            return logit_loss(target_logits, targets, "sigmoid", self.__device_metrics.block(states.device))
        target_logits = linear(states)          # CPU tensors: the reference's own operator order
        with torch.no_grad():
            predictions = torch.sigmoid(target_logits) >= 0.5
            true_positives = (predictions & targets).sum().float()
            false_positives = (predictions & (~targets)).sum().float()
            false_negatives = ((~predictions) & targets).sum().float()
            precision = true_positives / (true_positives + false_positives + 1e-10)
            recall = true_positives / (true_positives + false_negatives + 1e-10)
            fscore = 2 * precision * recall / (precision + recall + 1e-10)
            num_samples = int(predictions.shape[0])
            self.__sum_f1 += float(fscore) * num_samples
            self.__sum_pr += float(precision) * num_samples
            self.__sum_re += float(recall) * num_samples
            self.__num_samples += num_samples
        losses = nn.functional.binary_cross_entropy_with_logits(input=target_logits, target=targets.float(),
                                                                reduction="none")
        return losses.sum(dim=-1).mean()


class Graph2SeqModule(ModuleWithMetrics):
    """graph2seq/graph2seq.py:36-81: the GNN, the summariser that turns the nodes of a graph into the decoder's initial
    state, and the copying decoder over the states of the backbone nodes."""

    # `ptgnn_amd.sequence.GruCopyingDecoder.fused_loss` instead of the decoder's `forward`; any other decoder module is
    # called as the reference calls it.  profiles/graph2seq_notes.md holds the comparison behind the default.
    use_fused_loss = True

    def __init__(self, gnn: nn.Module, decoder: nn.Module, node_to_graph_representation: nn.Module):
        super().__init__()
        self._gnn = gnn
        self._decoder = decoder
        self.__node_to_graph_representation = node_to_graph_representation

    def _reset_module_metrics(self) -> None:
        self.__loss_sum = 0.0
        self.__num_mbs = 0
        self.__device_loss_sums = {}       # device -> float64 [] accumulator; dropped (no launch) on reset

    def _module_metrics(self) -> Dict[str, Any]:
        loss_sum = self.__loss_sum
        for acc in self.__device_loss_sums.values():       # the blocking reads: only here, where the reference reads too
            loss_sum += float(acc.cpu())
        return {"loss": loss_sum / self.__num_mbs}

    def _get_initial_decoder_states(self, gnn_output: GnnOutput):
        inputs, outputs = gnn_output.input_node_representations, gnn_output.output_node_representations
        if outputs.is_cuda:
            inputs, outputs = _f32(inputs), _f32(outputs)
        return self.__node_to_graph_representation(ElementsToSummaryRepresentationInput(
            element_embeddings=torch.cat((inputs, outputs), dim=-1),
            element_to_sample_map=gnn_output.node_to_graph_idx, num_samples=gnn_output.num_graphs))

    def __decoder_inputs(self, encoder_mb_data: Dict[str, Any]) -> Dict[str, Any]:
        """The GNN, the backbone gather and the summariser: what the decoder is given besides its own minibatch data."""
        gnn_output: GnnOutput = self._gnn(**encoder_mb_data)
        states = gnn_output.output_node_representations
        backbone = gnn_output.node_idx_references["backbone_nodes"]
        if not states.is_cuda:             # device dispatch: CPU tensors take the reference's own operator order
            memories = states[backbone]
        elif backbone.shape[0] == 0:       # no backbone nodes: nothing is launched
            memories = _f32(states).new_zeros(0, states.shape[1]) + _f32(states).sum() * 0.0
        else:
            memories = sequence._rows(_f32(states), backbone)
        return dict(input_memories=memories,
                    input_memories_origin_idx=gnn_output.node_graph_idx_reference["backbone_nodes"],
                    initial_states=self._get_initial_decoder_states(gnn_output))

    def forward(self, *, encoder_mb_data: Dict[str, Any], decoder_mb_data: Dict[str, Any]):
        decoder = self._decoder
        fused = self.use_fused_loss and isinstance(decoder, sequence.GruCopyingDecoder)
        loss = (decoder.fused_loss if fused else decoder)(**self.__decoder_inputs(encoder_mb_data), **decoder_mb_data)
        with torch.no_grad():
            if loss.is_cuda:               # no call of forward waits for the device
                acc = self.__device_loss_sums.get(loss.device)
                if acc is None:
                    self.__device_loss_sums[loss.device] = loss.detach().double()
                else:
                    acc.add_(loss.detach())
            else:
                self.__loss_sum += float(loss.detach())
            self.__num_mbs += 1
        return loss

    def greedy_decode(self, *, encoder_mb_data: Dict[str, Any], input_element_ids, start_id: int, end_id: int,
                      max_seq_len: int, top_k: int = 100, early_exit: int = 0):
        """graph2seq.py:175-204 without the host loop: the decoder inputs exactly as `forward` forms them, under
        torch.no_grad(), handed to `sequence.GruCopyingDecoder.greedy_decode` (its argument and result conventions,
        `early_exit` included; `input_element_ids` has one id per backbone node)."""
        with torch.no_grad():
            return self._decoder.greedy_decode(**self.__decoder_inputs(encoder_mb_data), input_element_ids=input_element_ids,
                                               start_id=start_id, end_id=end_id, max_seq_len=max_seq_len, top_k=top_k,
                                               early_exit=early_exit)

    def beam_decode(self, *, encoder_mb_data: Dict[str, Any], input_element_ids, start_id: int, end_id: int,
                    max_seq_len: int, beam_width: int, top_k: int = 100):
        """Beam search on the decoder inputs `greedy_decode` forms, handed to `sequence.GruCopyingDecoder.beam_decode`
        (its argument and result conventions: the `beam_width` best sequences of every sample)."""
        with torch.no_grad():
            return self._decoder.beam_decode(**self.__decoder_inputs(encoder_mb_data), input_element_ids=input_element_ids,
                                             start_id=start_id, end_id=end_id, max_seq_len=max_seq_len,
                                             beam_width=beam_width, top_k=top_k)

    def beam_decode_finishing(self, *, encoder_mb_data: Dict[str, Any], input_element_ids, start_id: int, end_id: int,
                              max_seq_len: int, beam_width: int, top_k: int = 100, length_penalty: float = 0.0,
                              early_exit: int = 0):
        """`beam_decode` with the decoder's `length_penalty` and `early_exit` (sequence.GruCopyingDecoder.beam_decode:
        GNMT length normalisation, leaving the loop once every hypothesis has finished), on the same decoder inputs.  A
        method of its own: the keyword list of `beam_decode` is pinned."""
        with torch.no_grad():
            return self._decoder.beam_decode(**self.__decoder_inputs(encoder_mb_data), input_element_ids=input_element_ids,
                                             start_id=start_id, end_id=end_id, max_seq_len=max_seq_len,
                                             beam_width=beam_width, top_k=top_k, length_penalty=length_penalty,
                                             early_exit=early_exit)

    def forward_sharded(self, *args, **kwargs):
        """The decoder attends over all memories of a sample: there is no sharded form."""
        raise PtgnnAmdError("forward_sharded: cannot combine partial pools of Graph2SeqModule")
