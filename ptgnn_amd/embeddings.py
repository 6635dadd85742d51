"""The node embedders every model of the reference starts its forward with (graphneuralnetwork.py:160): mirrors of
ptgnn/neuralmodels/embeddings/strelementrepresentationmodel.py:16-142 (`TokenUnitEmbedder`, `SubtokenUnitEmbedder`,
`CnnConfig`, `CharUnitEmbedder`: same class names, constructor keywords, submodule creation order, initialisers,
`embedding_layer` property, forward signatures and name-mangled parameter names, so a reference state_dict loads strictly and the same seed gives the same initial
values).  `StrElementRepresentationModel` -- vocabulary, tensorisation, minibatching -- works unchanged around them
(a subclass overriding `build_neural_module`).

GPU route:
  * TokenUnitEmbedder: the HIP row gather (backward: the deterministic segment sum over a plan of the token ids), dropout;
  * SubtokenUnitEmbedder: the fused embedding bag (csrc/embedding_bag.hip) as one autograd node -- no [B, S, D] tensor, the
    table gradient a deterministic segment sum over the bag's plan, `arg` kept for max -- then the HIP Linear of the
    output layer and dropout;
  * CharUnitEmbedder: the first convolution over the one-hot input as one fused table sum (csrc/char_conv.hip: no one_hot,
    no [B, L, C] tensor), the second and third as windowed Linears on the exact-fp32 MFMA GEMMs over channel-last row
    frames (char_cnn.py: a Conv1d is a Linear whose rows overlap, forward and backward), the HIP window max, dropout.
    Filter counts or an embedding size that are not multiples of 4, and char tables beyond the char-embed range, compose
    the same sequence from the embedding bag (or the row gather), copied windows through `dense.linear` and the window max.
  * LinearFeatureEmbedder (linearmapembedding.py:13-29, the node embedder of the PPI model): `dense.linear`, with Tanh / ReLU
    in the GEMM epilogue where the fused node takes the widths and any other activation module applied after.
Shapes beyond the bag's range (D not a multiple of 4, more than 32 subtokens) compose the reference's operator sequence
from the HIP row gather and torch elementwise arithmetic.  CPU tensors take the reference's own operator order on torch
(device dispatch as in every layer of the package); fp16 / bf16 tables are up-cast on entry and the result cast back.
"""
import math
from typing import NamedTuple, Optional

import torch
from torch import nn

from ptgnn_amd import _lib, char_cnn, dense, ops, torch_route
from ptgnn_amd.sequence import _rows

_HALF = (torch.float16, torch.bfloat16)


def _check_ids(what: str, table: torch.Tensor, *index) -> None:
    for t in index:
        if not t.is_cuda or t.dtype != torch.int64:
            raise _lib.PtgnnAmdError(f"{what}: the ids and lengths of a GPU table must be CUDA int64 tensors (got "
                                     f"{t.dtype} on {t.device})")


class _EmbeddingBag(torch.autograd.Function):
    """sum / mean / max of table[ids[b, s]] over s < lengths[b] on the fused HIP bag; backward = the segment sum over the
    bag's plan (ops.embedding_bag_backward), routed by the saved `arg` for max."""

    @staticmethod
    def forward(ctx, table, ids, lengths, kind):
        need_grad = ctx.needs_input_grad[0]
        res = ops.embedding_bag(table, ids, lengths, kind, return_arg=need_grad and kind == "max")
        out, arg = res if isinstance(res, tuple) else (res, None)
        ctx.save_for_backward(ids, lengths, arg)
        ctx.kind, ctx.rows = kind, table.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        ids, lengths, arg = ctx.saved_tensors
        return ops.embedding_bag_backward(g.contiguous(), ids, lengths, ctx.kind, ctx.rows, arg=arg), None, None, None


def embedding_bag(table: torch.Tensor, ids: torch.Tensor, lengths: torch.Tensor, kind: str) -> torch.Tensor:
    """Differentiable (w.r.t. `table`) subtoken pool on the HIP kernels; `ops.embedding_bag_supported(D, S)` shapes only."""
    return _EmbeddingBag.apply(table.contiguous(), ids, lengths, kind)


def _composed_pool(table: torch.Tensor, ids: torch.Tensor, lengths: torch.Tensor, kind: str) -> torch.Tensor:
    """strelementrepresentationmodel.py:67-82 on the HIP row gather plus torch elementwise arithmetic, for shapes outside
    the fused bag.  Dead slots read row 0 (their ids may be anything) and are masked out."""
    B, S = ids.shape
    live = torch.arange(S, device=ids.device).unsqueeze(0) < lengths.unsqueeze(-1)            # [B, S]
    flat = torch.where(live, ids, torch.zeros_like(ids)).clamp_(0, table.shape[0] - 1).reshape(-1)
    embedded = _rows(table, flat).reshape(B, S, table.shape[1])
    if kind == "max":
        return embedded.masked_fill(~live.unsqueeze(-1), -math.inf).max(dim=-2)[0]
    pooled = (embedded * live.unsqueeze(-1).float()).sum(dim=-2)
    return pooled / (lengths.unsqueeze(-1).float() + 1e-10) if kind == "mean" else pooled


class TokenUnitEmbedder(nn.Module):
    def __init__(self, vocabulary_size: int, embedding_size: int, dropout_rate: float):
        super().__init__()
        self.__embeddings = nn.Embedding(num_embeddings=vocabulary_size, embedding_dim=embedding_size)
        nn.init.xavier_uniform_(self.__embeddings.weight)
        self.__dropout_layer = nn.Dropout(p=dropout_rate)

    @property
    def embedding_layer(self) -> nn.Embedding:
        return self.__embeddings

    def forward(self, token_idxs: torch.Tensor) -> torch.Tensor:
        """:param token_idxs: [B] token ids;  :return: [B, D]"""
        table = self.__embeddings.weight
        if not table.is_cuda:             # device dispatch: CPU tensors take the reference's own operator order
            return self.__dropout_layer(self.__embeddings(token_idxs))
        _check_ids("TokenUnitEmbedder", table, token_idxs)
        rows = _rows(table.float(), token_idxs.reshape(-1)).reshape(*token_idxs.shape, table.shape[1])
        return self.__dropout_layer(rows.to(table.dtype))


class SubtokenUnitEmbedder(nn.Module):
    def __init__(self, vocabulary_size: int, embedding_size: int, dropout_rate: float, subtoken_combination_kind: str,
                 use_dense_output: bool = True):
        super().__init__()
        assert subtoken_combination_kind in {"mean", "max", "sum"}
        self.__subtoken_combination_kind = subtoken_combination_kind
        self.__embeddings = nn.Embedding(num_embeddings=vocabulary_size, embedding_dim=embedding_size)
        nn.init.uniform_(self.__embeddings.weight)
        if use_dense_output:
            self.__out_layer = nn.Linear(embedding_size, embedding_size, bias=False)
            nn.init.xavier_uniform_(self.__out_layer.weight)
        else:
            self.__out_layer = None
        self.__dropout_layer = nn.Dropout(p=dropout_rate)

    @property
    def embedding_layer(self) -> nn.Embedding:
        return self.__embeddings

    def __device_forward(self, token_idxs, lengths):
        table, kind = self.__embeddings.weight, self.__subtoken_combination_kind
        _check_ids("SubtokenUnitEmbedder", table, token_idxs, lengths)
        if token_idxs.dim() != 2 or lengths.shape != token_idxs.shape[:1]:
            raise _lib.PtgnnAmdError(f"SubtokenUnitEmbedder: token_idxs {tuple(token_idxs.shape)} / lengths "
                                     f"{tuple(lengths.shape)} are not [B, max_num_subtokens] / [B]")
        dt = table.dtype
        if dt not in _HALF and dt != torch.float32:
            raise _lib.PtgnnAmdError(f"SubtokenUnitEmbedder: no kernel for a {dt} table")
        table32 = table.float()           # AMP tables: fp32 inside, the table's dtype outside
        if ops.embedding_bag_supported(table.shape[1], token_idxs.shape[1]):
            pooled = embedding_bag(table32, token_idxs, lengths, kind)
        else:
            pooled = _composed_pool(table32, token_idxs, lengths, kind)
        drop = self.__dropout_layer
        if self.__out_layer is None:
            return drop(pooled.to(dt))
        weight = self.__out_layer.weight.float()
        out = dense.linear_act_dropout(pooled, weight, None, None, drop.p, self.training)
        if out is None:
            out = drop(dense.linear(pooled, weight))
        return out.to(dt)

    def forward(self, token_idxs: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """
        :param token_idxs: The subtoken ids in a [B, max_num_subtokens] matrix.
        :param lengths: A [B]-sized vector containing the lengths
        :return: a [B, D] matrix of D-sized representations, one per input example.
        """
        if self.__embeddings.weight.is_cuda:
            return self.__device_forward(token_idxs, lengths)
        embedded = torch_route.subtoken_embed(token_idxs, lengths, self.__embeddings.weight,
                                              self.__subtoken_combination_kind)
        if self.__out_layer is not None:
            embedded = self.__out_layer(embedded)
        return self.__dropout_layer(embedded)


class CnnConfig(NamedTuple):
    l1_filters: int
    l1_window_size: int
    l2_filters: int
    l2_window_size: int
    lout_window_size: int


def _conv_as_linear(weight: torch.Tensor) -> torch.Tensor:
    """A Conv1d weight [F, C_in, w] as the [F, w * C_in] matrix of the windowed Linear (column k C_in + c = W[:, c, k]);
    differentiable, so the gradient lands in Conv1d layout by autograd."""
    return weight.permute(0, 2, 1).reshape(weight.shape[0], -1)


class CharUnitEmbedder(nn.Module):
    def __init__(self, num_chars: int, embedding_size: int, config: CnnConfig, dropout_rate: float = 0.0):
        super().__init__()
        self.__num_chars_in_vocabulary = num_chars
        self.__conv_l1 = nn.Conv1d(in_channels=num_chars, out_channels=config.l1_filters,
                                   kernel_size=config.l1_window_size)
        self.__conv_l2 = nn.Conv1d(in_channels=config.l1_filters, out_channels=config.l2_filters,
                                   kernel_size=config.l2_window_size)
        self.__conv_l3 = nn.Conv1d(in_channels=config.l2_filters, out_channels=embedding_size,
                                   kernel_size=config.lout_window_size, bias=False)
        self.__dropout = nn.Dropout(p=dropout_rate)

    def __windowed(self, chars, table, b1, w2, b2, w3, k1, k2, k3):
        """Row frames (char_cnn.py): one char-embed launch, two windowed GEMMs, one window max."""
        B, L = chars.shape
        R, pad = L - k1 + 1, char_cnn.frame_pad(k2, k3)
        a1 = char_cnn.char_window_embed(chars, table, b1, k1, pad)
        a2 = char_cnn.window_linear(a1, _conv_as_linear(w2), b2, k2, pad, B * R, act="relu")
        l3 = char_cnn.window_linear(a2, _conv_as_linear(w3), None, k3, pad, B * R)
        return char_cnn.window_max(l3, pad, B, R, R - k2 - k3 + 2)

    def __composed(self, chars, table, b1, w2, b2, w3, k1, k2, k3):
        """The same sequence from the existing operators: window ids through the embedding bag (sum), windows materialised
        by a copy in front of `dense.linear`, the HIP window max."""
        B, L = chars.shape
        C, R = self.__num_chars_in_vocabulary, L - k1 + 1
        taps = torch.arange(k1, device=chars.device) * C
        ids = (chars.clamp(0, C - 1).unfold(1, k1, 1) + taps).reshape(B * R, k1)
        lengths = torch.full((B * R,), k1, dtype=torch.int64, device=chars.device)
        if ops.embedding_bag_supported(table.shape[1], k1):
            pooled = embedding_bag(table, ids, lengths, "sum")
        else:
            pooled = _composed_pool(table, ids, lengths, "sum")
        act, rows = torch.relu(pooled + b1), R
        for weight, bias, k, relu in ((w2, b2, k2, True), (w3, None, k3, False)):
            width = act.shape[1]
            windows = act.reshape(B, rows, width).unfold(1, k, 1).permute(0, 1, 3, 2).reshape(-1, k * width)
            rows = rows - k + 1
            act = dense.linear(windows, _conv_as_linear(weight).contiguous(), bias)
            act = torch.relu(act) if relu else act
        return char_cnn.window_max(act, 0, B, rows, rows)

    def __device_forward(self, chars):
        w1, b1 = self.__conv_l1.weight, self.__conv_l1.bias
        w2, b2, w3 = self.__conv_l2.weight, self.__conv_l2.bias, self.__conv_l3.weight
        if not chars.is_cuda or chars.dtype != torch.int64 or chars.dim() != 2:
            raise _lib.PtgnnAmdError(f"CharUnitEmbedder: chars must be a CUDA int64 [B, max_num_chars] tensor (got "
                                     f"{tuple(chars.shape)} {chars.dtype} on {chars.device})")
        dt = w1.dtype
        if dt not in _HALF and dt != torch.float32:
            raise _lib.PtgnnAmdError(f"CharUnitEmbedder: no kernel for {dt} parameters")
        k1, k2, k3 = w1.shape[2], w2.shape[2], w3.shape[2]
        if chars.shape[1] < k1 + k2 + k3 - 2:
            raise _lib.PtgnnAmdError(f"CharUnitEmbedder: {chars.shape[1]} chars are fewer than the {k1 + k2 + k3 - 2} that "
                                     f"windows of {k1}, {k2}, {k3} need for one output position")
        C, F1, F2, D = self.__num_chars_in_vocabulary, w1.shape[0], w2.shape[0], w3.shape[0]
        # AMP parameters: fp32 inside, the parameters' dtype outside
        table = w1.float().permute(2, 1, 0).reshape(k1 * C, F1)      # row k C + c = W1[:, c, k]
        args = (chars, table, b1.float(), w2.float(), b2.float(), w3.float(), k1, k2, k3)
        # the weight-gradient GEMMs read float4 rows of both operands: F1, F2 and D in fours
        if F1 % 4 == 0 and F2 % 4 == 0 and D % 4 == 0 and ops.char_embed_supported(C, k1, F1):
            summary = self.__windowed(*args)
        else:
            summary = self.__composed(*args)
        return self.__dropout(summary.to(dt))

    def forward(self, chars):
        """
        :param chars: [B, max_num_chars]
        :return: [B, D]
        """
        if self.__conv_l1.weight.is_cuda:
            return self.__device_forward(chars)
        summary = torch_route.char_cnn(chars, self.__num_chars_in_vocabulary, self.__conv_l1, self.__conv_l2,
                                       self.__conv_l3)                  # CPU tensors: the reference's operator order
        return self.__dropout(summary)


class LinearFeatureEmbedder(nn.Module):
    def __init__(self, input_element_size: int, output_embedding_size: int, activation: Optional[nn.Module] = None):
        super().__init__()
        self.__linear_map = nn.Linear(input_element_size, output_embedding_size, bias=False)
        nn.init.xavier_uniform_(self.__linear_map.weight)
        self.__activation = activation

    def forward(self, features):
        weight, act = self.__linear_map.weight, self.__activation
        if not features.is_cuda:          # device dispatch: CPU tensors take the reference's own operator order
            mapped_features = self.__linear_map(features)
            return act(mapped_features) if act is not None else mapped_features
        dt = features.dtype
        if (dt not in _HALF and dt != torch.float32) or features.dim() != 2:
            raise _lib.PtgnnAmdError(f"LinearFeatureEmbedder: features must be a 2-D float matrix (got "
                                     f"{tuple(features.shape)} {dt})")
        x, w = features.float(), weight.float()           # AMP: fp32 inside, the features' dtype outside
        fused = {nn.Tanh: "tanh", nn.ReLU: "relu"}.get(type(act))
        if fused is not None and x.shape[0] > 0:
            out = dense.linear_act_dropout(x, w, None, fused, 0.0, False)
            if out is not None:
                return out.to(dt)
        if x.shape[0] == 0:
            mapped_features = x.new_zeros(0, w.shape[0])
        else:
            mapped_features = dense.linear(x, w)
        if act is not None:
            mapped_features = act(mapped_features)
        return mapped_features.to(dt)
