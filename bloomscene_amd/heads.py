"""The three anchor MLP heads of ``generate_neural_gaussians`` on the MI355X: ``mlp_opacity`` (Tanh), ``mlp_cov`` and
``mlp_color`` (Sigmoid) of ``scene/gaussian_model.py:234-252`` on the visible anchors, with the view geometry of
``gaussian_renderer/__init__.py:151-154`` ("GR"), the reshapes of GR:171/181/185 and the offset mask of GR:172, in HIP
behind ``include/bloomscene_heads.h``.

    neural_opacity, color, scale_rot = anchor_heads(feat, anchor, viewpoint_camera.camera_center, pc.get_opacity_mlp,
                                                    pc.get_cov_mlp, pc.get_color_mlp, offset_mask=binary_grid_masks)
    ... = anchor_heads_tensors(feat, anchor, camera_center, weights, K, offset_mask=None)     # the same over 12 tensors
    heads = AnchorHeads(pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp, feat=..., ...)   # views.training_view(heads=)

The function and its gradient are written out in the header.  One kernel forward; the backward recomputes the hidden layer
from the inputs (the header's chain gives the same bits, so the ReLU gate agrees), so the forward keeps the inputs and the
color output only.  ``feat`` is read in place through its row stride (a ``torch.split`` or ``index_select`` result costs no
copy where its column stride is 1); the weights are read where ``nn.Linear`` keeps them, live, with no packed copy.
Weight gradients are bit-identical from run to run; they, and their scratch, are only paid for when a weight requires a
gradient.  Everything runs on the current torch stream without a host synchronisation (capturable into a CUDA graph) and
takes its scratch from torch's allocator.  There is no CPU path; importing this module needs no GPU.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from . import _operands as _ops
from ._operands import ptr

MAX_F, MAX_K = 64, 16                  # BSR_HEADS_MAX_F, BSR_HEADS_MAX_K
HEAD_NAMES = ("mlp_opacity", "mlp_cov", "mlp_color")
HEAD_OUTPUTS = (1, 7, 3)               # outputs per offset
HEAD_LAST = (nn.Tanh, None, nn.Sigmoid)
WEIGHT_NAMES = tuple(f"{h}.{t}" for h in HEAD_NAMES for t in ("W1", "b1", "W2", "b2"))


def _pointers(tensors):
    return _capi.HeadsPointers(*[ptr(t) for t in tensors])


def head_weights(mlp_opacity, mlp_cov, mlp_color):
    """The twelve parameters of the three ``nn.Sequential`` heads, (W1, b1, W2, b2) per head, as they are (live).  Each head
    must be ``Linear, ReLU, Linear`` followed by ``Tanh`` (opacity), nothing (cov), ``Sigmoid`` (color); anything else
    raises NotImplementedError naming the layer."""
    out = []
    for name, mlp, last in zip(HEAD_NAMES, (mlp_opacity, mlp_cov, mlp_color), HEAD_LAST):
        out += _ops.sequential_weights("anchor_heads", name, mlp, last)
    return out


class _Heads(torch.autograd.Function):
    """inputs: feat, anchor, camera_center, mask (or None), K, want_maps, then the twelve weights."""

    @staticmethod
    def forward(ctx, feat, anchor, cam, mask, K, want_maps, *weights):
        n, F = feat.shape
        dev = feat.device
        opacity = torch.empty(n * K, 1, dtype=torch.float32, device=dev)
        color = torch.empty(n * K, 3, dtype=torch.float32, device=dev)
        scale_rot = torch.empty(n * K, 7, dtype=torch.float32, device=dev)
        maps = torch.empty(n * (3 * F + 11 * K), dtype=torch.float32, device=dev) if want_maps else None
        if n > 0:
            _capi.call("bsr_anchor_heads_forward", n, F, K, ptr(feat), _ops.row_stride(feat, n, F), ptr(anchor),
                       ptr(cam), ptr(mask), _pointers(weights), ptr(opacity), ptr(color), ptr(scale_rot), ptr(maps),
                       _ops.stream(dev))
        ctx.save_for_backward(feat, anchor, cam, mask, color, *weights)
        ctx.K = K
        ctx.set_materialize_grads(False)
        if want_maps:
            ctx.mark_non_differentiable(maps)
            return opacity, color, scale_rot, maps
        return opacity, color, scale_rot

    @staticmethod
    @once_differentiable
    def backward(ctx, g_opacity, g_color, g_scale_rot, *_):
        feat, anchor, cam, mask, color = ctx.saved_tensors[:5]
        weights = ctx.saved_tensors[5:]
        n, F = feat.shape
        K = ctx.K
        dev = feat.device
        need = ctx.needs_input_grad

        g_opacity, g_color, g_scale_rot = (_ops.as_f32_contiguous(g) for g in (g_opacity, g_color, g_scale_rot))
        d_feat = torch.empty(n, F, dtype=torch.float32, device=dev) if need[0] else None
        d_anchor = torch.empty(n, 3, dtype=torch.float32, device=dev) if need[1] else None
        d_mask = torch.empty(n, K, dtype=torch.float32, device=dev) if mask is not None and need[3] else None
        d_weights = [torch.empty_like(w, memory_format=torch.contiguous_format) if need[6 + i] else None
                     for i, w in enumerate(weights)]
        sums = any(d is not None for d in d_weights)
        scratch = None
        if sums and n > 0:
            scratch = _ops.scratch(_capi.lib().bsr_anchor_heads_scratch_bytes(n, F, K), dev)
        if n > 0 or sums:
            _capi.call("bsr_anchor_heads_backward", n, F, K, ptr(feat), _ops.row_stride(feat, n, F), ptr(anchor),
                       ptr(cam), ptr(mask), _pointers(weights), ptr(color), ptr(g_opacity), ptr(g_color),
                       ptr(g_scale_rot), ptr(d_feat), ptr(d_anchor), ptr(d_mask),
                       _pointers(d_weights) if sums else None, ptr(scratch), _ops.stream(dev))
        return (d_feat, d_anchor, None, d_mask, None, None, *d_weights)


def _checked(who, feat, anchor, camera_center, weights, K, offset_mask):
    """The header's operands from the caller's tensors, checked in ``_operands``' order of complaints."""
    weights = list(weights)
    if len(weights) != 12:
        raise ValueError(f"{who}: weights must be the twelve tensors {', '.join(WEIGHT_NAMES)} (got {len(weights)})")
    tensors = [("feat", feat), ("anchor", anchor), ("camera_center", camera_center)]
    if offset_mask is not None:
        tensors.append(("offset_mask", offset_mask))
    tensors += list(zip(WEIGHT_NAMES, weights))
    _ops.check_tensors(who, tensors)
    if camera_center.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{who}: camera_center requires a gradient; the heads give none to the camera")
    if isinstance(K, bool) or not isinstance(K, int):
        raise ValueError(f"{who}: K must be an int (got {K!r})")
    if feat.dim() != 2:
        raise ValueError(f"{who}: feat must be [n, F] (got {list(feat.shape)})")
    n, F = feat.shape
    if not 1 <= F <= MAX_F:
        raise ValueError(f"{who}: F = feat.shape[1] must be in [1, {MAX_F}] (got {F})")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: K must be in [1, {MAX_K}] (got {K})")
    if n * max(7 * K, F + 4) >= 2 ** 31:
        raise ValueError(f"{who}: n * max(7 K, F + 4) must be below 2^31 (got n = {n})")
    if tuple(anchor.shape) != (n, 3):
        raise ValueError(f"{who}: anchor must be [{n}, 3] (got {list(anchor.shape)})")
    if camera_center.numel() != 3:
        raise ValueError(f"{who}: camera_center must hold 3 values (got {list(camera_center.shape)})")
    if offset_mask is not None:
        if tuple(offset_mask.shape) not in ((n, K, 1), (n, K), (n * K, 1)):
            raise ValueError(f"{who}: offset_mask must be [{n}, {K}, 1], [{n}, {K}] or [{n * K}, 1] (got {list(offset_mask.shape)})")
        offset_mask = offset_mask.reshape(n, K).contiguous()
    for h, outputs in enumerate(HEAD_OUTPUTS):
        shapes = ((F, F + 4), (F,), (outputs * K, F), (outputs * K,))
        for i, shape in enumerate(shapes):
            if tuple(weights[4 * h + i].shape) != shape:
                raise ValueError(f"{who}: {WEIGHT_NAMES[4 * h + i]} must be {list(shape)} for F = {F}, K = {K} "
                                 f"(got {list(weights[4 * h + i].shape)})")
    _ops.check_on_gpu(who, tensors)
    _ops.check_same_device(who, tensors, feat.device)
    feat = _ops.rows_in_place(feat, n, F)
    weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
    return feat, anchor.contiguous(), camera_center.detach().reshape(3).contiguous(), offset_mask, weights


def anchor_heads_tensors(feat, anchor, camera_center, weights, K, offset_mask=None):
    """The heads over raw tensors: ``feat [n, F]``, ``anchor [n, 3]``, ``camera_center [3]`` (a device tensor, never read on
    the host, no gradient), ``weights`` the twelve tensors (W1 ``[F, F + 4]``, b1 ``[F]``, W2 ``[O, F]``, b2 ``[O]``) of
    opacity, cov, color with ``O = K, 7 K, 3 K``, ``offset_mask [n, K, 1]``, ``[n, K]`` or ``[n K, 1]``.
    -> ``(neural_opacity [n K, 1], color [n K, 3], scale_rot [n K, 7])``, differentiable in ``feat``, ``anchor``,
    ``offset_mask`` and the weights."""
    feat, anchor, cam, mask, weights = _checked("anchor_heads_tensors", feat, anchor, camera_center, weights, K, offset_mask)
    return _Heads.apply(feat, anchor, cam, mask, K, False, *weights)


def anchor_heads(feat, anchor, camera_center, mlp_opacity, mlp_cov, mlp_color, offset_mask=None):
    """GR:151-154 and GR:168-185 (``use_feat_bank=False``) in one call; the three ``mlp_*`` are the model's ``nn.Sequential``
    heads, whose parameters are read live.  ``K`` is ``mlp_opacity``'s output width.  See ``anchor_heads_tensors``."""
    who = "anchor_heads"
    tensors = [("feat", feat), ("anchor", anchor), ("camera_center", camera_center)]
    if offset_mask is not None:
        tensors.append(("offset_mask", offset_mask))
    _ops.check_tensors(who, tensors)
    weights = head_weights(mlp_opacity, mlp_cov, mlp_color)
    K = int(weights[2].shape[0])
    feat, anchor, cam, mask, weights = _checked(who, feat, anchor, camera_center, weights, K, offset_mask)
    return _Heads.apply(feat, anchor, cam, mask, K, False, *weights)


@torch.no_grad()
def anchor_heads_maps(feat, anchor, camera_center, weights, K, offset_mask=None):
    """The forward's pre-activations, for measurement (no gradient): ``(neural_opacity, color, scale_rot, pre1 [n, 3 F],
    pre2 [n, 11 K])`` -- ``pre1`` head-major, ``pre2`` with K columns of opacity, 7 K of cov, 3 K of color."""
    feat, anchor, cam, mask, weights = _checked("anchor_heads_maps", feat, anchor, camera_center, weights, K, offset_mask)
    n, F = feat.shape
    opacity, color, scale_rot, maps = _Heads.apply(feat, anchor, cam, mask, K, True, *weights)
    return opacity, color, scale_rot, maps[:n * 3 * F].view(n, 3 * F), maps[n * 3 * F:].view(n, 11 * K)


class AnchorHeads:
    """The three heads as ``views.training_view``'s ``heads=`` argument: a callable that holds the three modules and the
    per-anchor tensors they read, and gathers ``feat``, ``anchor`` and the mask by ``idx`` itself:

        heads = AnchorHeads(pc.get_opacity_mlp, pc.get_cov_mlp, pc.get_color_mlp, feat=feat, anchor=anchor,
                            camera_center=cam.camera_center, offset_mask=grid_masks)
        out = training_view(cam, anchor, scaling, rotation, offsets, heads, bg)          # calls heads(idx)

    ``offset_mask [N, K, 1]`` (GR:43) is optional.  ``bind(feat, anchor, camera_center, offset_mask=None)`` returns a copy
    holding other tensors (a new view every iteration); ``evaluate(feat, anchor, camera_center, offset_mask=None)`` is
    ``anchor_heads`` on tensors that are gathered already."""

    def __init__(self, mlp_opacity, mlp_cov, mlp_color, feat=None, anchor=None, camera_center=None, offset_mask=None):
        head_weights(mlp_opacity, mlp_cov, mlp_color)   # (refuse an unsupported head here, not in the first step)
        self.mlp_opacity, self.mlp_cov, self.mlp_color = mlp_opacity, mlp_cov, mlp_color
        self.feat, self.anchor, self.camera_center, self.offset_mask = feat, anchor, camera_center, offset_mask

    def evaluate(self, feat, anchor, camera_center, offset_mask=None):
        return anchor_heads(feat, anchor, camera_center, self.mlp_opacity, self.mlp_cov, self.mlp_color, offset_mask=offset_mask)

    def bind(self, feat, anchor, camera_center, offset_mask=None):
        return AnchorHeads(self.mlp_opacity, self.mlp_cov, self.mlp_color, feat, anchor, camera_center, offset_mask)

    def __call__(self, idx):
        if self.feat is None or self.anchor is None or self.camera_center is None:
            raise ValueError("AnchorHeads: called with an index list but feat, anchor and camera_center are not bound "
                             "(give them to the constructor or to bind())")
        mask = None if self.offset_mask is None else self.offset_mask.index_select(0, idx)
        return self.evaluate(self.feat.index_select(0, idx), self.anchor.index_select(0, idx), self.camera_center, mask)
