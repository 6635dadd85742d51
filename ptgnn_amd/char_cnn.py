"""Autograd nodes of the char-CNN embedder (embeddings.CharUnitEmbedder) on ROW FRAMES.

Every activation and gradient matrix of the trunk is channel-last with R = L - k1 + 1 rows per sample -- sample b at rows
[pad + b R, pad + (b + 1) R) of a [pad + B R + pad, C] buffer, pad = max(k2, k3) - 1 -- so that

  * a Conv1d is a Linear whose input rows overlap: the window at row r is the w * C_in contiguous floats that start at row
    r (ops.window_linear), and its weight gradient the same split-row GEMM over those rows (ops.window_weight_grad);
  * its input gradient is again a windowed Linear: row r reads the gradient rows r - (w - 1) .. r against the tap-flipped
    weight, and the zero rows between two samples' valid positions are the zero padding a transposed convolution needs.

Invariants: in a GRADIENT frame the pad rows and every row past a layer's valid positions (P2 = R - k2 + 1 after the second
convolution, P3 = P2 - k3 + 1 after the third) are exact zeros -- `_WindowMax` writes them so, a bias-free windowed Linear
of zero rows and the ReLU mask keep them so.  In an ACTIVATION frame the pad rows are zeroed and the rows past the valid
positions hold finite junk: they only ever meet zero gradient rows in the weight gradient (an uninitialised pad could
hold a NaN, and 0 * NaN would poison it).  A valid output row never reads a junk row: position p < P2 of the second
convolution reads a1 rows up to P1 - 1, p < P3 of the third a2 rows up to P2 - 1.
"""
import torch

from ptgnn_amd import ops


def frame_pad(k2: int, k3: int) -> int:
    return max(int(k2), int(k3)) - 1


def _new_frame(pad: int, rows: int, width: int, device) -> torch.Tensor:
    """An uninitialised [pad + rows + pad, width] frame whose pad rows are zero."""
    frame = torch.empty(2 * pad + rows, width, dtype=torch.float32, device=device)
    if pad:
        frame[:pad].zero_()
        frame[pad + rows:].zero_()
    return frame


def _flipped(weight: torch.Tensor, window: int) -> torch.Tensor:
    """The tap-flipped transpose of a [F, w * C] windowed weight: [C, w * F] with column j F + f = weight[f, (w - 1 - j) C
    + c].  Built once per backward: the windowed weight is itself rebuilt from the Conv1d parameter in every forward."""
    n_out = weight.shape[0]
    return weight.detach().reshape(n_out, window, -1).flip(1).permute(2, 1, 0).reshape(-1, window * n_out).contiguous()


class _CharWindowEmbed(torch.autograd.Function):
    """The a1 frame: relu(bias + sum_k table[k C + chars[b, p + k]]) on the fused HIP table sum (ops.char_embed); backward =
    the deterministic chunked LDS accumulation (ops.char_embed_backward)."""

    @staticmethod
    def forward(ctx, chars, table, bias, window, pad):
        B, L = chars.shape
        rows = B * (L - window + 1)
        frame = _new_frame(pad, rows, table.shape[1], table.device)
        ops.char_embed(chars, table, bias, window, act="relu", out=frame, out_first_row=pad)
        ctx.save_for_backward(chars, frame)
        ctx.dims = (window, pad, rows, table.shape[0] // window, bias is not None)
        return frame

    @staticmethod
    def backward(ctx, g):
        chars, frame = ctx.saved_tensors
        window, pad, rows, num_chars, has_bias = ctx.dims
        g = g.contiguous()
        want_b = has_bias and ctx.needs_input_grad[2]
        d_table, d_bias = ops.char_embed_backward(g[pad:pad + rows], frame[pad:pad + rows], chars, num_chars, window,
                                                  act="relu", want_bias=want_b)
        return None, d_table, d_bias, None, None


class _WindowLinear(torch.autograd.Function):
    """y frame = act(W . x[r .. r + w - 1] + b) over the `rows` interior rows of the x frame (ops.window_linear, the ReLU in
    the GEMM's epilogue).  Backward: the ReLU mask through ops.act_dropout_backward, d x = the windowed Linear of the
    masked gradient frame offset by -(w - 1) rows against the tap-flipped weight, d W (and d b) = ops.window_weight_grad."""

    @staticmethod
    def forward(ctx, x, weight, bias, window, pad, rows, act):
        y = _new_frame(pad, rows, weight.shape[0], x.device)
        ops.window_linear(x, pad, rows, window, weight, bias, act=act, out=y, out_first_row=pad)
        ctx.save_for_backward(x, weight, y if act is not None else None)
        ctx.dims = (window, pad, rows, act, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        window, pad, rows, act, has_bias = ctx.dims
        g = g.contiguous()
        if act is not None:
            masked = _new_frame(pad, rows, g.shape[1], g.device)
            ops.act_dropout_backward(g[pad:pad + rows], y[pad:pad + rows], None, 1.0, act, out=masked[pad:pad + rows])
            g = masked
        d_x = d_w = d_b = None
        if ctx.needs_input_grad[0]:
            d_x = _new_frame(pad, rows, x.shape[1], g.device)
            ops.window_linear(g, pad - (window - 1), rows, window, _flipped(weight, window), out=d_x, out_first_row=pad)
        want_b = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            res = ops.window_weight_grad(x, pad, rows, window, g[pad:pad + rows], want_bias=want_b)
            d_w, d_b = res if want_b else (res, None)
        elif want_b:
            d_b = g[pad:pad + rows].sum(dim=0)
        return d_x, d_w, d_b, None, None, None, None


class _WindowMax(torch.autograd.Function):
    """[B, D] = max over the first `valid` of every sample's R frame rows, the lowest position on a tie (ops.window_max);
    backward writes the whole gradient frame: the winner row per (sample, column), exact zeros elsewhere and in the pads."""

    @staticmethod
    def forward(ctx, x, pad, num_samples, rows_per_sample, valid):
        need = ctx.needs_input_grad[0]
        res = ops.window_max(x, pad, num_samples, rows_per_sample, valid, return_arg=need)
        out, arg = res if need else (res, None)
        ctx.save_for_backward(arg)
        ctx.dims = (pad, num_samples, rows_per_sample)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        pad, num_samples, rows_per_sample = ctx.dims
        frame = _new_frame(pad, num_samples * rows_per_sample, g.shape[1], g.device)
        ops.window_max_backward(g.contiguous(), arg, rows_per_sample, out=frame, out_first_row=pad)
        return frame, None, None, None, None


def char_window_embed(chars, table, bias, window: int, pad: int) -> torch.Tensor:
    return _CharWindowEmbed.apply(chars, table.contiguous(), bias, int(window), int(pad))


def window_linear(x, weight, bias, window: int, pad: int, rows: int, act=None) -> torch.Tensor:
    return _WindowLinear.apply(x, weight.contiguous(), bias, int(window), int(pad), int(rows), act)


def window_max(x, pad: int, num_samples: int, rows_per_sample: int, valid: int) -> torch.Tensor:
    return _WindowMax.apply(x, int(pad), int(num_samples), int(rows_per_sample), int(valid))
