"""The rate term of BloomScene's loss on the MI355X: ``Entropy_gaussian`` / ``Low_bound`` (``utils/entropy_models.py:10-50``,
"EM") and the selection, masking and sums ``gaussian_renderer/__init__.py:100-127`` ("GR") wraps around its three calls,
in HIP behind ``include/bloomscene_entropy.h``.

    bits = gaussian_bits(x, mean, scale, Q, x_mean=None)                        # EM:14-31, [n, C]
    pc.entropy_gaussian = EntropyGaussian()                                      # the drop-in module, same forward()
    total, count = rate_sum(x, mean, scale, Q, x_mean, rows=None, weight=None, weight_repeat=1)
    bit_per_param, bit_per_feat, bit_per_scaling, bit_per_offsets = context_rates(...)   # GR:77-84, 100-127

The function and its gradient are written out in the header.  One kernel forward, one backward that recomputes the
elementwise terms from the operands; ``x``, ``mean``, ``scale`` are read in place through their row stride (the
``torch.split`` views of GR:77-78 cost no copy).  ``rate_sum`` takes GR's ``choose_idx`` as a mask: no ``nonzero``, no
gather, no host read, and its sums are bit-identical from run to run.  ``x_mean`` stays on the device.  Everything runs on
the current torch stream without a host synchronisation (capturable into a CUDA graph) and takes its scratch from torch's
allocator.  There is no CPU path.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _capi
from . import _operands as _ops
from ._operands import ptr, row_stride

Q_SINGLE, Q_ROW, Q_ELEMENT = 0, 1, 2     # BSR_ENTROPY_Q_* of the header
G_DENSE, G_SINGLE = 0, 1                 # BSR_ENTROPY_G_*


class _Operands:
    """The checked operands of one call: tensors the kernels can read as they are, and the shape.  Every dtype
    (TypeError) before any device (ValueError); "on the GPU" is checked before the shapes here, "on one device" after
    them (``_operands`` names this exception to its order)."""

    def __init__(self, who, x, mean, scale, Q, x_mean, rows=None, weight=None, weight_repeat=1):
        tensors = [("x", x), ("mean", mean), ("scale", scale)]
        if isinstance(Q, torch.Tensor):
            tensors.append(("Q", Q))
        elif not isinstance(Q, (int, float)):
            raise TypeError(f"{who}: Q must be a number or a torch.Tensor (got {type(Q).__name__})")
        if isinstance(x_mean, torch.Tensor):
            tensors.append(("x_mean", x_mean))
        elif x_mean is not None and not isinstance(x_mean, (int, float)):
            raise TypeError(f"{who}: x_mean must be a 0-dim torch.Tensor, a number or None (got {type(x_mean).__name__})")
        if weight is not None:
            tensors.append(("weight", weight))
        if rows is not None:
            _ops.check_tensors(who, [("rows", rows)], torch.bool)
        _ops.check_tensors(who, tensors)
        _ops.check_on_gpu(who, tensors + ([("rows", rows)] if rows is not None else []))
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"{who}: x must be [n, C] with C >= 1 (got {list(x.shape)})")
        n, C = x.shape
        for name, t in (("mean", mean), ("scale", scale)):
            if tuple(t.shape) != (n, C):
                raise ValueError(f"{who}: {name} must be [{n}, {C}] like x (got {list(t.shape)})")
        r = int(weight_repeat)
        if r < 1 or C % r != 0:
            raise ValueError(f"{who}: weight_repeat must divide C = {C} (got {weight_repeat})")
        if weight is None and r != 1:
            raise ValueError(f"{who}: weight_repeat = {r} without a weight")
        if n >= 2 ** 31 or n * C >= 2 ** 40:
            raise ValueError(f"{who}: need n below 2^31 and n * C below 2^40 (got {n} * {C})")
        dev = x.device
        if isinstance(Q, torch.Tensor):
            if Q.numel() == 1:
                self.q_mode, q = Q_SINGLE, Q.reshape(1)
            elif tuple(Q.shape) in ((n, 1), (n,)):
                self.q_mode, q = Q_ROW, Q.reshape(n)
            elif tuple(Q.shape) == (n, C):
                self.q_mode, q = Q_ELEMENT, Q
            else:
                raise ValueError(f"{who}: Q must be a scalar, [{n}, 1] or [{n}, {C}] (got {list(Q.shape)})")
            self.q = q.contiguous()
        else:
            self.q_mode = Q_SINGLE
            self.q = torch.full((1,), float(Q), dtype=torch.float32, device=dev)
        if x_mean is None:
            x_mean = x.detach().mean() if n > 0 else torch.zeros((), dtype=torch.float32, device=dev)   # EM:19
        elif not isinstance(x_mean, torch.Tensor):
            x_mean = torch.full((), float(x_mean), dtype=torch.float32, device=dev)
        if x_mean.numel() != 1:
            raise ValueError(f"{who}: x_mean must hold one value (got {list(x_mean.shape)})")
        self.x_mean = x_mean.detach().reshape(1)   # (EM:22 detaches the bounds)
        if rows is not None:
            if tuple(rows.shape) != (n,):
                raise ValueError(f"{who}: rows must be [{n}] (got {list(rows.shape)})")
            rows = rows.contiguous().view(torch.uint8)
        if weight is not None:
            if tuple(weight.shape) != (n, C // r):
                raise ValueError(f"{who}: weight must be [{n}, {C // r}] (got {list(weight.shape)})")
            weight = weight.contiguous()
        for t in (mean, scale, self.q, self.x_mean, rows, weight):
            if t is not None and t.device != dev:
                raise ValueError(f"{who}: every operand must be on {dev} (got {t.device})")
        self.n, self.C, self.r = n, C, r
        self.x, self.mean, self.scale = (_ops.rows_in_place(t, n, C) for t in (x, mean, scale))
        self.rows, self.weight = rows, weight


def _scratch(n, C, r, device):
    return _ops.scratch(_capi.lib().bsr_entropy_scratch_bytes(n, C, r), device)


def _forward(n, C, r, x, mean, scale, q, q_mode, x_mean, rows, weight, bits=None, likelihood=None, total=None, count=None):
    sums = total is not None or count is not None
    scratch = _scratch(n, C, r, x.device) if sums else None
    _capi.call("bsr_entropy_forward", n, C, r, ptr(x), row_stride(x, n, C), ptr(mean), row_stride(mean, n, C),
               ptr(scale), row_stride(scale, n, C), ptr(q), q_mode, ptr(x_mean), ptr(rows), ptr(weight), ptr(bits),
               ptr(likelihood), ptr(total), ptr(count), ptr(scratch), _ops.stream(x.device))


def _backward(ctx, g, g_mode):
    """One bsr_entropy_backward for the saved operands -> (dx, dmean, dscale, dq, dw), None where not needed."""
    x, mean, scale, q, x_mean, rows, weight = ctx.saved_tensors
    n, C, r, q_mode = ctx.shape
    need = ctx.needs_input_grad
    dev = x.device

    def out(wanted, *shape):
        return torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None

    dx, dmean, dscale = out(need[0], n, C), out(need[1], n, C), out(need[2], n, C)
    dq = out(need[3], *{Q_SINGLE: (1,), Q_ROW: (n,), Q_ELEMENT: (n, C)}[q_mode])
    dw = out(weight is not None and need[6], n, C // r)
    scratch = _scratch(n, C, r, dev) if dq is not None and q_mode == Q_SINGLE else None
    _capi.call("bsr_entropy_backward", n, C, r, ptr(x), row_stride(x, n, C), ptr(mean), row_stride(mean, n, C),
               ptr(scale), row_stride(scale, n, C), ptr(q), q_mode, ptr(x_mean), ptr(rows), ptr(weight), ptr(g), g_mode,
               ptr(dx), ptr(dmean), ptr(dscale), ptr(dq), ptr(dw), ptr(scratch), _ops.stream(dev))
    return dx, dmean, dscale, dq, dw


class _Rate(torch.autograd.Function):
    """inputs: x, mean, scale, q, x_mean, rows, weight (tensor positions 0-6), then r, q_mode, want_sum."""

    @staticmethod
    def forward(ctx, x, mean, scale, q, x_mean, rows, weight, r, q_mode, want_sum):
        n, C = x.shape
        ctx.save_for_backward(x, mean, scale, q, x_mean, rows, weight)
        ctx.shape = (n, C, r, q_mode)
        ctx.want_sum = want_sum
        if want_sum:
            total = torch.empty((), dtype=torch.float32, device=x.device)
            count = torch.empty((), dtype=torch.int64, device=x.device)
            _forward(n, C, r, x, mean, scale, q, q_mode, x_mean, rows, weight, total=total, count=count)
            ctx.mark_non_differentiable(count)
            return total, count
        bits = torch.empty(n, C, dtype=torch.float32, device=x.device)
        if n > 0:
            _forward(n, C, r, x, mean, scale, q, q_mode, x_mean, rows, weight, bits=bits)
        return bits

    @staticmethod
    def backward(ctx, g, *_):
        dx, dmean, dscale, dq, dw = _backward(ctx, _ops.as_f32_contiguous(g), G_SINGLE if ctx.want_sum else G_DENSE)
        return dx, dmean, dscale, dq, None, None, dw, None, None, None


def _apply(op, want_sum):
    # (op.q is a reshape of the caller's Q: autograd carries the kernel's gradient back to Q's own shape)
    return _Rate.apply(op.x, op.mean, op.scale, op.q, op.x_mean, op.rows, op.weight, op.r, op.q_mode, want_sum)


def gaussian_bits(x, mean, scale, Q, x_mean=None):
    """EM:14-31: ``-log2`` of the probability the Gaussian ``(mean, scale)`` gives the bin of width ``Q`` around ``x``,
    floored at 1e-6.  ``x``, ``mean``, ``scale`` float32 ``[n, C]`` on the GPU; ``Q`` a number or a tensor (one value,
    ``[n, 1]`` or ``[n, C]``); ``x_mean`` a 0-dim device tensor (never read on the host) or None for ``x.mean()``.
    -> ``bits`` float32 ``[n, C]``, differentiable in ``x``, ``mean``, ``scale`` and a tensor ``Q``."""
    return _apply(_Operands("gaussian_bits", x, mean, scale, Q, x_mean), False)


@torch.no_grad()
def gaussian_likelihood(x, mean, scale, Q, x_mean=None):
    """The likelihood ``l`` of the header BEFORE its floor, float32 ``[n, C]`` (for measurement: no gradient)."""
    op = _Operands("gaussian_likelihood", x, mean, scale, Q, x_mean)
    out = torch.empty(op.n, op.C, dtype=torch.float32, device=x.device)
    if op.n > 0:
        _forward(op.n, op.C, 1, op.x, op.mean, op.scale, op.q, op.q_mode, op.x_mean, None, None, likelihood=out)
    return out


def rate_sum(x, mean, scale, Q, x_mean, rows=None, weight=None, weight_repeat=1):
    """The sum of ``gaussian_bits`` over the rows chosen by the bool mask ``rows [n]`` (GR:100-113 without the gathers),
    each column ``j`` times ``weight[i, j // weight_repeat]`` where a weight ``[n, C / weight_repeat]`` is given
    (GR:114, GR:120).  -> ``total`` float32 0-dim and ``count`` int64 0-dim on the device (chosen rows * C, the
    ``numel()`` of GR:123-127).  Differentiable in ``x``, ``mean``, ``scale``, ``Q`` and ``weight``; the gradients are
    dense and zero in the rows not chosen."""
    return _apply(_Operands("rate_sum", x, mean, scale, Q, x_mean, rows, weight, weight_repeat), True)


class EntropyGaussian(nn.Module):
    """``Entropy_gaussian`` of EM:10-31 on the MI355X: same constructor, same ``forward`` arguments."""

    def __init__(self, Q=1):
        super().__init__()
        self.Q = Q

    def forward(self, x, mean, scale, Q=None, x_mean=None):
        return gaussian_bits(x, mean, scale, self.Q if Q is None else Q, x_mean)


def context_rates(feat, grid_scaling, grid_offsets, context, choose, grid_masks, mask_anchor_rate, feat_mean,
                  scaling_mean, offsets_mean, feat_dim, n_offsets, q_feat=0.25, q_scaling=2.5e-4, q_offsets=5e-2, steps=None):
    """GR:77-84 and GR:100-127 over three ``rate_sum`` calls.  ``steps``: the step sizes ``Q [n, 3]`` (columns feat,
    scaling, offsets) that ``context.context_head`` returned beside ``context``; with it GR:82-84 are not evaluated again
    (and ``q_*`` are not read).

    ``feat [n, feat_dim]``, ``grid_scaling [n, 6]``, ``grid_offsets [n, n_offsets, 3]`` (after the noise of GR:91-97);
    ``context [n, 2 feat_dim + 12 + 6 n_offsets + 3]`` the grid MLP's output (GR:76); ``choose`` bool ``[n]`` (GR:100-101);
    ``grid_masks [n, n_offsets, 1]`` (GR:43); ``mask_anchor_rate`` (GR:46); the three ``*_mean`` 0-dim device tensors of
    GR:117-119; ``q_*`` the step sizes of GR:52-54.
    -> ``(bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param)`` of GR:123-127."""
    who = "context_rates"
    if context.dim() != 2 or context.shape[1] != 2 * feat_dim + 12 + 6 * n_offsets + 3:
        raise ValueError(f"{who}: context must be [n, {2 * feat_dim + 12 + 6 * n_offsets + 3}] (got {list(context.shape)})")
    n = context.shape[0]
    mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, adj_feat, adj_scaling, adj_offsets = \
        torch.split(context, [feat_dim, feat_dim, 6, 6, 3 * n_offsets, 3 * n_offsets, 1, 1, 1], dim=-1)    # GR:77-78
    if steps is None:
        Q_feat = q_feat * (1 + torch.tanh(adj_feat))                                                        # GR:82-84
        Q_scaling = q_scaling * (1 + torch.tanh(adj_scaling))
        Q_offsets = q_offsets * (1 + torch.tanh(adj_offsets))
    else:
        _ops.check_tensors(who, [("steps", steps)], None)
        if tuple(steps.shape) != (n, 3):
            raise ValueError(f"{who}: steps must be [{n}, 3] (got {list(steps.shape)})")
        Q_feat, Q_scaling, Q_offsets = steps[:, 0:1], steps[:, 1:2], steps[:, 2:3]
    sum_feat, n_feat = rate_sum(feat, mean, scale, Q_feat, feat_mean, rows=choose)                          # GR:117
    sum_scaling, n_scaling = rate_sum(grid_scaling, mean_scaling, scale_scaling, Q_scaling, scaling_mean, rows=choose)
    sum_offsets, n_offsets_el = rate_sum(grid_offsets.reshape(n, 3 * n_offsets), mean_offsets, scale_offsets, Q_offsets,
                                         offsets_mean, rows=choose, weight=grid_masks.reshape(n, n_offsets),
                                         weight_repeat=3)                                                   # GR:119-120
    bit_per_feat_param = sum_feat / n_feat * mask_anchor_rate                                               # GR:123-127
    bit_per_scaling_param = sum_scaling / n_scaling * mask_anchor_rate
    bit_per_offsets_param = sum_offsets / n_offsets_el * mask_anchor_rate
    bit_per_param = (sum_feat + sum_scaling + sum_offsets) / (n_feat + n_scaling + n_offsets_el) * mask_anchor_rate
    return bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param
