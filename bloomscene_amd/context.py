"""The context model's head of ``generate_neural_gaussians`` on the MI355X: the grid MLP ``mlp_grid``
(``scene/gaussian_model.py:254-258``) on the hash-grid encoding of the visible anchors, the three adaptive step sizes of
``gaussian_renderer/__init__.py:82-84`` ("GR"), and either the noise injection of training (GR:87-97) or the
``STE_multistep`` quantiser of rendering (GR:140-142), in HIP behind ``include/bloomscene_context.h``.

    context, Q, feat, grid_scaling, grid_offsets = context_head(enc, pc.get_grid_mlp, F, K, feat=feat,
        grid_scaling=grid_scaling, grid_offsets=grid_offsets, noise=(randn_like(feat), randn_like(...), randn_like(...)))
    ... = context_head_tensors(enc, (W1, b1, W2, b2), F, K, ...)                       # the same over the four tensors
    feat, grid_scaling, grid_offsets = context_quantise(enc, pc.get_grid_mlp, F, K, feat, grid_scaling, grid_offsets,
                                                        pc._anchor_feat.mean(), pc.get_scaling.mean(), pc._offset.mean())
    head = ContextHead(pc.get_grid_mlp, F, K);  head(enc, ...);  head.quantise(enc, ...)

The function and its gradient are written out in the header.  One kernel forward; the backward recomputes the hidden layer
and the three adjustment columns from the inputs (the header's chains give the same bits, so the ReLU gate agrees), so the
forward keeps the encoding and the noise only.  ``enc`` and the attributes are read in place through their row stride; the
weights are read where ``nn.Linear`` keeps them, live.  The noise is the caller's ``torch.randn_like``: no random number
is drawn here.  The quantiser evaluates three of layer 2's rows, writes no ``context`` and has no gradient.  Weight
gradients are bit-identical from run to run; they, and their scratch, are only paid for when a weight requires a gradient.
Everything runs on the current torch stream without a host synchronisation (capturable into a CUDA graph) and takes its
scratch from torch's allocator.  There is no CPU path; importing this module needs no GPU.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from . import _operands as _ops
from ._operands import ptr, row_stride

MAX_D, MAX_H, MAX_F, MAX_K = 128, 128, 64, 16     # BSR_CONTEXT_MAX_*
Q_DEFAULT = (0.25, 2.5e-4, 5e-2)                  # GR:52-54: feat, scaling, offsets
WEIGHT_NAMES = ("mlp_grid.W1", "mlp_grid.b1", "mlp_grid.W2", "mlp_grid.b2")
ATTRIBUTES = ("feat", "grid_scaling", "grid_offsets")


def outputs(F, K):
    """The width of ``context``: the split of GR:77-78."""
    return 2 * F + 12 + 6 * K + 3


def _pointers(tensors):
    return _capi.ContextPointers(*[ptr(t) for t in tensors])


def grid_weights(mlp_grid):
    """The four parameters (W1, b1, W2, b2) of the ``nn.Sequential`` grid MLP, as they are (live).  It must be ``Linear,
    ReLU, Linear`` with biases; anything else raises NotImplementedError naming the layer."""
    return _ops.sequential_weights("context_head", "mlp_grid", mlp_grid)


def _steps(q):
    return float(q[0]), float(q[1]), float(q[2])


class _Context(torch.autograd.Function):
    """inputs: enc, the three attributes [n, C] (or None), their three noises (or None), F, K, q, want_maps, the four weights."""

    @staticmethod
    def forward(ctx, enc, feat, scaling, offsets, noise_feat, noise_scaling, noise_offsets, F, K, q, want_maps, *weights):
        n, D = enc.shape
        H, O = weights[0].shape[0], outputs(F, K)
        dev = enc.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        context, Q = new(n, O), new(n, 3)
        xs, noises, widths = (feat, scaling, offsets), (noise_feat, noise_scaling, noise_offsets), (F, 6, 3 * K)
        outs = [None if x is None else new(n, C) for x, C in zip(xs, widths)]
        maps = new(n, H) if want_maps else None
        if n > 0:
            strided = [a for x, C in zip(xs, widths) for a in (ptr(x), 0 if x is None else row_stride(x, n, C))]
            _capi.call("bsr_context_head_forward", n, D, H, F, K, ptr(enc), row_stride(enc, n, D), _pointers(weights),
                       *q, *strided, *[ptr(t) for t in noises], ptr(context), ptr(Q), *[ptr(t) for t in outs],
                       ptr(maps), _ops.stream(dev))
        ctx.save_for_backward(enc, noise_feat, noise_scaling, noise_offsets, *weights)
        ctx.shape = (F, K, q)
        ctx.set_materialize_grads(False)
        if want_maps:
            ctx.mark_non_differentiable(maps)
            return (context, Q, *outs, maps)
        return (context, Q, *outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_context, g_Q, g_feat, g_scaling, g_offsets, *_):
        enc = ctx.saved_tensors[0]
        noises = ctx.saved_tensors[1:4]
        weights = ctx.saved_tensors[4:]
        F, K, q = ctx.shape
        n, D = enc.shape
        H = weights[0].shape[0]
        dev = enc.device
        need = ctx.needs_input_grad

        g_outs = [g_feat, g_scaling, g_offsets]
        d_xs = [g if need[1 + c] else None for c, g in enumerate(g_outs)]        # the gradient to x is the upstream itself
        g_context, g_Q = _ops.as_f32_contiguous(g_context), _ops.as_f32_contiguous(g_Q)
        g_outs = [_ops.as_f32_contiguous(g) for g in g_outs]
        d_enc, d_weights = None, [None] * 4
        if any(g is not None for g in [g_context, g_Q] + g_outs):
            d_enc = torch.empty(n, D, dtype=torch.float32, device=dev) if need[0] else None
            d_weights = [torch.empty_like(w, memory_format=torch.contiguous_format) if need[11 + i] else None
                         for i, w in enumerate(weights)]
            sums = any(d is not None for d in d_weights)
            scratch = None
            if sums and n > 0:
                scratch = _ops.scratch(_capi.lib().bsr_context_scratch_bytes(n, D, H, F, K), dev)
            if (n > 0 and (sums or d_enc is not None)) or sums:
                _capi.call("bsr_context_head_backward", n, D, H, F, K, ptr(enc), row_stride(enc, n, D),
                           _pointers(weights), *q, *[ptr(t) for t in noises], ptr(g_context), ptr(g_Q),
                           *[ptr(g) for g in g_outs], ptr(d_enc), _pointers(d_weights) if sums else None, ptr(scratch),
                           _ops.stream(dev))
        return (d_enc, *d_xs, None, None, None, None, None, None, None, *d_weights)


def _checked(who, enc, weights, F, K, xs, noise=None, means=None, q=Q_DEFAULT):
    """The header's operands from the caller's tensors, checked in ``_operands``' order of complaints.  ``xs`` = (feat,
    grid_scaling, grid_offsets), each a tensor or None; ``noise`` (the training form) a 3-tuple beside it or None;
    ``means`` (the quantiser) the three scalars.  -> enc, weights, xs as [n, C] rows the kernels can read, noises, means,
    q, the shape grid_offsets came in."""
    weights = list(weights) if isinstance(weights, (list, tuple)) else [weights]
    if noise is None:
        noise = (None, None, None)
    if not isinstance(noise, (list, tuple)) or len(noise) != 3:
        raise ValueError(f"{who}: noise must be a 3-tuple (feat, grid_scaling, grid_offsets), with None for an absent attribute")
    tensors = [("enc", enc)]
    tensors += [(name, x) for name, x in zip(ATTRIBUTES, xs) if x is not None]
    tensors += [(f"noise[{c}] ({name})", t) for c, (name, t) in enumerate(zip(ATTRIBUTES, noise)) if t is not None]
    if means is not None:
        tensors += [(f"{name}_mean", m) for name, m, x in zip(("feat", "scaling", "offsets"), means, xs) if x is not None]
    tensors += list(zip(WEIGHT_NAMES, weights))
    _ops.check_tensors(who, tensors)
    if torch.is_grad_enabled():
        for c, t in enumerate(noise):
            if t is not None and t.requires_grad:
                raise NotImplementedError(f"{who}: noise[{c}] ({ATTRIBUTES[c]}) requires a gradient; the head gives none to the noise")
    if len(weights) != 4:
        raise ValueError(f"{who}: weights must be the four tensors {', '.join(WEIGHT_NAMES)} (got {len(weights)})")
    for name, v in (("F", F), ("K", K)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{who}: {name} must be an int (got {v!r})")
    try:
        if len(q) != 3:
            raise ValueError
        q = _steps(q)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: q must be three numbers (feat, scaling, offsets) (got {q!r})") from None
    if enc.dim() != 2:
        raise ValueError(f"{who}: enc must be [n, D] (got {list(enc.shape)})")
    n, D = enc.shape
    if not 1 <= D <= MAX_D:
        raise ValueError(f"{who}: D = enc.shape[1] must be in [1, {MAX_D}] (got {D})")
    if weights[0].dim() != 2:
        raise ValueError(f"{who}: {WEIGHT_NAMES[0]} must be [H, {D}] (got {list(weights[0].shape)})")
    H = weights[0].shape[0]
    if not 1 <= H <= MAX_H:
        raise ValueError(f"{who}: H = {WEIGHT_NAMES[0]}.shape[0] must be in [1, {MAX_H}] (got {H})")
    if not 1 <= F <= MAX_F:
        raise ValueError(f"{who}: F must be in [1, {MAX_F}] (got {F})")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: K must be in [1, {MAX_K}] (got {K})")
    O = outputs(F, K)
    if n * max(O, D) >= 2 ** 31:
        raise ValueError(f"{who}: n * max(2 F + 12 + 6 K + 3, D) must be below 2^31 (got n = {n})")
    for name, w, shape in zip(WEIGHT_NAMES, weights, ((H, D), (H,), (O, H), (O,))):
        if tuple(w.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)} for D = {D}, H = {H}, F = {F}, K = {K} (got {list(w.shape)})")
    accepted = (((n, F),), ((n, 6),), ((n, K, 3), (n, 3 * K)))
    rows, noises, offsets_shape = [], [], None
    for c, (name, x, t, shapes, C) in enumerate(zip(ATTRIBUTES, xs, noise, accepted, (F, 6, 3 * K))):
        if x is None:
            if t is not None:
                raise ValueError(f"{who}: noise[{c}] is given but {name} is not")
            rows.append(None)
            noises.append(None)
            continue
        if tuple(x.shape) not in shapes:
            raise ValueError(f"{who}: {name} must be {' or '.join(str(list(s)) for s in shapes)} (got {list(x.shape)})")
        if c == 2:
            offsets_shape = tuple(x.shape)
        if means is None:
            if t is None:
                raise ValueError(f"{who}: {name} is given without noise[{c}] (the caller's torch.randn_like({name}))")
            if t.numel() != n * C or tuple(t.shape) not in shapes:
                raise ValueError(f"{who}: noise[{c}] must be shaped like {name} (got {list(t.shape)})")
            noises.append(t.detach().reshape(n, C).contiguous())
        else:
            noises.append(None)
        rows.append(x.reshape(n, C))
    if means is not None:
        means = list(means)
        for c, (name, m) in enumerate(zip(("feat", "scaling", "offsets"), means)):
            if rows[c] is None:
                means[c] = None
            elif m.numel() != 1:
                raise ValueError(f"{who}: {name}_mean must hold one value (got {list(m.shape)})")
    _ops.check_on_gpu(who, tensors)
    _ops.check_same_device(who, tensors, enc.device)
    enc = _ops.rows_in_place(enc, n, D)
    rows = [None if x is None else _ops.rows_in_place(x, n, C) for x, C in zip(rows, (F, 6, 3 * K))]
    weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
    if means is not None:
        means = [None if m is None else m.detach().reshape(1) for m in means]
    return enc, weights, rows, noises, means, q, offsets_shape


def _head(who, enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, q, want_maps):
    enc, weights, xs, noises, _, q, offsets_shape = _checked(who, enc, weights, F, K, (feat, grid_scaling, grid_offsets),
                                                             noise=noise, q=q)
    out = list(_Context.apply(enc, *xs, *noises, F, K, q, want_maps, *weights))
    if out[4] is not None:
        out[4] = out[4].reshape(offsets_shape)
    return tuple(out)


def context_head_tensors(enc, weights, F, K, feat=None, grid_scaling=None, grid_offsets=None, noise=None, q=Q_DEFAULT):
    """GR:76-97 over raw tensors: ``enc [n, D]`` the encoding, ``weights`` = (W1 ``[H, D]``, b1 ``[H]``, W2 ``[O, H]``, b2
    ``[O]``) with ``O = 2 F + 12 + 6 K + 3``; optionally ``feat [n, F]``, ``grid_scaling [n, 6]``, ``grid_offsets [n, K, 3]``
    with ``noise`` = the three ``torch.randn_like`` tensors of GR:91-93 (None for an absent attribute); ``q`` the base step
    sizes of GR:52-54.
    -> ``(context [n, O], Q [n, 3], feat', grid_scaling', grid_offsets')``: the grid MLP's output (GR:76), the step sizes of
    GR:82-84 as columns feat, scaling, offsets, and the noised attributes of GR:95-97 (None where absent; ``grid_offsets'``
    in the shape it came in).  One autograd node, differentiable in ``enc``, the attributes and the weights."""
    return _head("context_head_tensors", enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, q, False)


def _module_call(who, mlp_grid, tensors):
    _ops.check_tensors(who, [(name, t) for name, t in tensors if t is not None])
    return grid_weights(mlp_grid)


def context_head(enc, mlp_grid, F, K, feat=None, grid_scaling=None, grid_offsets=None, noise=None, q=Q_DEFAULT):
    """``context_head_tensors`` over the model's ``nn.Sequential`` (``pc.get_grid_mlp``), whose parameters are read live."""
    who = "context_head"
    weights = _module_call(who, mlp_grid, [("enc", enc), ("feat", feat), ("grid_scaling", grid_scaling), ("grid_offsets", grid_offsets)])
    return _head(who, enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, q, False)


@torch.no_grad()
def context_head_maps(enc, weights, F, K, feat=None, grid_scaling=None, grid_offsets=None, noise=None, q=Q_DEFAULT):
    """``context_head_tensors`` and the hidden pre-activations, for measurement (no gradient): ``(context, Q, feat',
    grid_scaling', grid_offsets', pre1 [n, H])``."""
    return _head("context_head_maps", enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, q, True)


@torch.no_grad()
def _quantise(who, enc, weights, F, K, feat, grid_scaling, grid_offsets, means, q, want_steps):
    enc, weights, xs, _, means, q, offsets_shape = _checked(who, enc, weights, F, K, (feat, grid_scaling, grid_offsets),
                                                            means=means, q=q)
    n, D = enc.shape
    H = weights[0].shape[0]
    dev = enc.device
    widths = (F, 6, 3 * K)
    outs = [None if x is None else torch.empty(n, C, dtype=torch.float32, device=dev) for x, C in zip(xs, widths)]
    Q = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_steps else None
    if n > 0:
        strided = [a for x, C in zip(xs, widths) for a in (ptr(x), 0 if x is None else row_stride(x, n, C))]
        _capi.call("bsr_context_quantise_forward", n, D, H, F, K, ptr(enc), row_stride(enc, n, D), _pointers(weights),
                   *q, *strided, *[ptr(m) for m in means], ptr(Q), *[ptr(t) for t in outs], _ops.stream(dev))
    if outs[2] is not None:
        outs[2] = outs[2].reshape(offsets_shape)
    return (*outs, Q) if want_steps else tuple(outs)


def context_quantise_tensors(enc, weights, F, K, feat, grid_scaling, grid_offsets, feat_mean, scaling_mean, offsets_mean,
                             q=Q_DEFAULT, steps=False):
    """GR:133-142 over raw tensors (see ``context_quantise``); ``steps=True`` also returns ``Q [n, 3]``."""
    return _quantise("context_quantise_tensors", enc, weights, F, K, feat, grid_scaling, grid_offsets,
                     (feat_mean, scaling_mean, offsets_mean), q, steps)


def context_quantise(enc, mlp_grid, F, K, feat, grid_scaling, grid_offsets, feat_mean, scaling_mean, offsets_mean, q=Q_DEFAULT):
    """GR:133-142 in one call: the step sizes from the last three rows of the grid MLP's second layer, then
    ``STE_multistep`` (clamp to ``mean +- 15000 Q``, round to the step, the soft part) on ``feat [n, F]``, ``grid_scaling
    [n, 6]`` and ``grid_offsets [n, K, 3]`` (None: left out).  The three means are 0-dim device tensors
    (``pc._anchor_feat.mean()`` ...), never read on the host.  -> the three quantised tensors, detached."""
    who = "context_quantise"
    weights = _module_call(who, mlp_grid, [("enc", enc), ("feat", feat), ("grid_scaling", grid_scaling), ("grid_offsets", grid_offsets)])
    return _quantise(who, enc, weights, F, K, feat, grid_scaling, grid_offsets, (feat_mean, scaling_mean, offsets_mean), q, False)


class ContextHead(nn.Module):
    """The grid MLP with its tails: ``forward`` is ``context_head`` (training, GR:76-97), ``quantise`` is
    ``context_quantise`` (rendering, GR:133-142).  Holds the model's own ``nn.Sequential``: its parameters are read live."""

    def __init__(self, mlp_grid, F, K, q=Q_DEFAULT):
        super().__init__()
        grid_weights(mlp_grid)   # (refuse an unsupported stack here, not in the first step)
        self.mlp_grid, self.F, self.K, self.q = mlp_grid, int(F), int(K), _steps(q)

    def forward(self, enc, feat=None, grid_scaling=None, grid_offsets=None, noise=None):
        return context_head(enc, self.mlp_grid, self.F, self.K, feat, grid_scaling, grid_offsets, noise, self.q)

    def quantise(self, enc, feat, grid_scaling, grid_offsets, feat_mean, scaling_mean, offsets_mean):
        return context_quantise(enc, self.mlp_grid, self.F, self.K, feat, grid_scaling, grid_offsets, feat_mean, scaling_mean,
                                offsets_mean, self.q)
