"""The two per-anchor blocks of a BloomScene training iteration that the visible-anchor index list drives, on the MI355X, in
HIP behind ``include/bloomscene_anchor_state.h``:

    # the prologue of generate_neural_gaussians, gaussian_renderer/__init__.py:34-46 ("GR")
    anchor, feat, grid_offsets, grid_scaling, binary_grid_masks, mask_anchor, mask_anchor_rate = visible(
        idx, pc._anchor, pc.x_bound_min, pc.x_bound_max, pc._anchor_feat, pc._offset, pc._scaling, pc._mask)

    # GaussianModel.training_statis, scene/gaussian_model.py:742-759 ("GM")
    accumulate(pc.opacity_accum, pc.anchor_demon, pc.offset_gradient_accum, pc.offset_denom,
               idx, neural_opacity, offset_selection_mask, radii, viewspace_point_tensor.grad)

``visible`` evaluates ``get_anchor`` (Quantize_anchor), ``get_scaling`` (exp), ``get_mask`` / ``get_mask_anchor`` (the sigmoid
straight-through binarisation) and ``mask_anchor_rate`` on the ``n`` visible rows only, in two launches; its backward writes
the dense ``[N, ...]`` gradients completely in one launch, each element by one thread (no float atomics: bit-identical
from run to run), and only those of inputs that require a gradient.  ``mask_anchor`` is bool already (``mask_anchor_bool``
of GR:45).  ``accumulate`` updates the four densification statistics in place in two launches.

``idx`` is int64 ``[n]`` on the device as ``GaussianRasterizer.visible_filter_indices`` returns it: STRICTLY ASCENDING and in
``[0, N)``.  A value out of range is never dereferenced (its row is zero and it contributes to nothing); ``check=True``
validates order and range with one host read and raises ValueError.  Without it nothing here waits on the host;
everything runs on the current torch stream and can be captured into a CUDA graph.  The function, its gradient and the
two deviations from the eager lines (the mask's forward value is exactly 0 / 1; the ``> 0.01`` decision is taken on the
library's sigmoid form) are written out in the header.  There is no CPU path; importing this module needs no GPU.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _capi
from . import _operands as _ops
from ._operands import ptr

MAX_F, MAX_K = 64, 16          # BSR_ANCHOR_STATE_MAX_F, BSR_ANCHOR_STATE_MAX_K
SCAN_BLOCK = 1024              # BSR_ANCHOR_STATE_SCAN


def _check_idx(who, idx, N):
    """Order and range of idx with ONE host read."""
    bad = (idx < 0).any() | (idx >= N).any()
    if idx.numel() > 1:
        bad = bad | (idx[1:] <= idx[:-1]).any()
    if bool(bad):
        raise ValueError(f"{who}: idx must be strictly ascending with every value in [0, {N})")


class _Visible(torch.autograd.Function):
    """inputs: idx, _anchor, bound_min, bound_max, _anchor_feat, _offset, _scaling, _mask (checked, dense but feat's rows)."""

    @staticmethod
    def forward(ctx, idx, anchor, bmin, bmax, feat, offset, scaling, mask):
        N, F = feat.shape
        K = offset.shape[1]
        n = idx.numel()
        dev = feat.device

        def new(*shape, dtype=torch.float32):
            return torch.empty(*shape, dtype=dtype, device=dev)

        o_anchor, o_feat, o_offsets, o_scaling = new(n, 3), new(n, F), new(n, K, 3), new(n, 6)
        o_masks, o_mask_anchor, o_rate = new(n, K, 1), new(n, dtype=torch.bool), new(())
        _capi.call("bsr_anchor_visible_forward", N, n, F, K, ptr(idx), ptr(anchor), ptr(bmin), ptr(bmax), ptr(feat),
                   _ops.row_stride(feat, N, F), ptr(offset), ptr(scaling), ptr(mask), ptr(o_anchor), ptr(o_feat),
                   ptr(o_offsets), ptr(o_scaling), ptr(o_masks), ptr(o_mask_anchor), ptr(o_rate), _ops.stream(dev))
        need = ctx.needs_input_grad
        ctx.save_for_backward(idx, mask if need[7] else None, o_scaling if need[6] else None)
        ctx.sizes = (N, F, K)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(o_mask_anchor, o_rate)
        return o_anchor, o_feat, o_offsets, o_scaling, o_masks, o_mask_anchor, o_rate

    @staticmethod
    @once_differentiable
    def backward(ctx, g_anchor, g_feat, g_offsets, g_scaling, g_masks, *_):
        idx, mask, grid_scaling = ctx.saved_tensors
        N, F, K = ctx.sizes
        n = idx.numel()
        dev = idx.device
        need = ctx.needs_input_grad

        def dense(wanted, *shape):
            return torch.empty(*shape, dtype=torch.float32, device=dev) if wanted else None

        ups = [_ops.as_f32_contiguous(g) for g in (g_anchor, g_feat, g_offsets, g_scaling, g_masks)]
        d_anchor, d_feat, d_offset = dense(need[1], N, 3), dense(need[4], N, F), dense(need[5], N, K, 3)
        d_scaling, d_mask = dense(need[6], N, 6), dense(need[7], N, K, 1)
        _capi.call("bsr_anchor_visible_backward", N, n, F, K, ptr(idx), ptr(mask), ptr(grid_scaling),
                   *[ptr(g) for g in ups], ptr(d_anchor), ptr(d_feat), ptr(d_offset), ptr(d_scaling), ptr(d_mask),
                   _ops.stream(dev))
        return None, d_anchor, None, None, d_feat, d_offset, d_scaling, d_mask


def visible(idx, _anchor, x_bound_min, x_bound_max, _anchor_feat, _offset, _scaling, _mask, check=False):
    """GR:34-46 on the rows ``idx`` (int64 ``[n]``, strictly ascending, in ``[0, N)``): ``_anchor [N, 3]``, the bounds ``[1, 3]``
    or ``[3]`` (device tensors, never read on the host, no gradient), ``_anchor_feat [N, F]`` (read through its row stride),
    ``_offset [N, K, 3]``, ``_scaling [N, 6]``, ``_mask [N, K, 1]``, all float32.
    -> ``(anchor [n, 3], feat [n, F], grid_offsets [n, K, 3], grid_scaling [n, 6], binary_grid_masks [n, K, 1],
    mask_anchor [n] bool, mask_anchor_rate 0-dim)``, differentiable in the five ``[N, ...]`` inputs.
    ``check=True`` validates ``idx`` with one host read (ValueError)."""
    who = "visible"
    f32 = torch.float32
    tensors = [("idx", idx, torch.int64), ("_anchor", _anchor, f32), ("x_bound_min", x_bound_min, f32),
               ("x_bound_max", x_bound_max, f32), ("_anchor_feat", _anchor_feat, f32), ("_offset", _offset, f32),
               ("_scaling", _scaling, f32), ("_mask", _mask, f32)]
    _ops.check_tensors(who, tensors, half_note=False)
    if torch.is_grad_enabled():
        for name, t, _ in tensors[2:4]:
            if t.requires_grad:
                raise NotImplementedError(f"{who}: {name} requires a gradient; Quantize_anchor gives none to the bounds")
    if idx.dim() != 1:
        raise ValueError(f"{who}: idx must be [n] (got {list(idx.shape)})")
    if _anchor_feat.dim() != 2:
        raise ValueError(f"{who}: _anchor_feat must be [N, F] (got {list(_anchor_feat.shape)})")
    N, F = _anchor_feat.shape
    if not 1 <= F <= MAX_F:
        raise ValueError(f"{who}: F = _anchor_feat.shape[1] must be in [1, {MAX_F}] (got {F})")
    if _offset.dim() != 3 or _offset.shape[0] != N or _offset.shape[2] != 3:
        raise ValueError(f"{who}: _offset must be [{N}, K, 3] (got {list(_offset.shape)})")
    K = _offset.shape[1]
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: K = _offset.shape[1] must be in [1, {MAX_K}] (got {K})")
    if N * max(F, 3 * K) >= 2 ** 31:
        raise ValueError(f"{who}: N * max(F, 3 K) must be below 2^31 (got N = {N})")
    if tuple(_anchor.shape) != (N, 3):
        raise ValueError(f"{who}: _anchor must be [{N}, 3] (got {list(_anchor.shape)})")
    if tuple(_scaling.shape) != (N, 6):
        raise ValueError(f"{who}: _scaling must be [{N}, 6] (got {list(_scaling.shape)})")
    if tuple(_mask.shape) not in ((N, K, 1), (N, K)):
        raise ValueError(f"{who}: _mask must be [{N}, {K}, 1] (got {list(_mask.shape)})")
    for name, t, _ in tensors[2:4]:
        if t.numel() != 3:
            raise ValueError(f"{who}: {name} must hold 3 values (got {list(t.shape)})")
    if idx.numel() > N:
        raise ValueError(f"{who}: idx holds {idx.numel()} rows, more than the {N} anchors")
    _ops.check_on_gpu(who, tensors)
    _ops.check_same_device(who, tensors, tensors[0][1].device)
    if check:
        _check_idx(who, idx, N)
    feat = _ops.rows_in_place(_anchor_feat, N, F)
    return _Visible.apply(idx.contiguous(), _anchor.contiguous(), x_bound_min.detach().reshape(3).contiguous(),
                          x_bound_max.detach().reshape(3).contiguous(), feat, _offset.contiguous(), _scaling.contiguous(),
                          _mask.reshape(N, K, 1).contiguous())


@torch.no_grad()
def accumulate(opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, idx, neural_opacity,
               offset_selection_mask, radii, viewspace_grad, check=False):
    """GM:743-759 in place: the accumulators ``[N, 1]``, ``[N, 1]``, ``[N K, 1]``, ``[N K, 1]`` (float32, contiguous),
    ``idx`` as for ``visible``, ``neural_opacity [n K, 1]``, ``offset_selection_mask`` bool ``[n K]``, ``radii`` int32 ``[M]``
    (the filter is ``radii > 0``; a bool ``[M]`` is taken as the filter itself) and ``viewspace_grad [M, 3]``, the ``.grad`` of
    the screen-space points.  Rows of ``radii`` / ``viewspace_grad`` beyond the selected count are ignored and selected
    candidates beyond ``M`` are skipped, so the padded form of ``render_anchors(capacity=)`` needs nothing special.
    Returns None."""
    who = "accumulate"
    if viewspace_grad is None:
        raise ValueError(f"{who}: viewspace_grad is None: pass viewspace_point_tensor.grad after the backward "
                         "(retain_grad() on a non-leaf)")
    f32 = torch.float32
    tensors = [("opacity_accum", opacity_accum, f32), ("anchor_demon", anchor_demon, f32),
               ("offset_gradient_accum", offset_gradient_accum, f32), ("offset_denom", offset_denom, f32),
               ("idx", idx, torch.int64), ("neural_opacity", neural_opacity, f32),
               ("offset_selection_mask", offset_selection_mask, torch.bool), ("radii", radii, (torch.int32, torch.bool)),
               ("viewspace_grad", viewspace_grad, f32)]
    _ops.check_tensors(who, tensors, half_note=False)
    if idx.dim() != 1:
        raise ValueError(f"{who}: idx must be [n] (got {list(idx.shape)})")
    n = idx.numel()
    N = opacity_accum.shape[0] if opacity_accum.dim() > 0 else -1
    if opacity_accum.dim() not in (1, 2) or opacity_accum.numel() != N:
        raise ValueError(f"{who}: opacity_accum must be [N, 1] (got {list(opacity_accum.shape)})")
    if anchor_demon.dim() not in (1, 2) or anchor_demon.shape[0] != N or anchor_demon.numel() != N:
        raise ValueError(f"{who}: anchor_demon must be [{N}, 1] (got {list(anchor_demon.shape)})")
    NK = offset_gradient_accum.numel()
    if offset_gradient_accum.dim() not in (1, 2) or offset_gradient_accum.shape[0] != NK or (N == 0) != (NK == 0) or \
            (N > 0 and NK % N != 0):
        raise ValueError(f"{who}: offset_gradient_accum must be [N K, 1] with N = {N} (got {list(offset_gradient_accum.shape)})")
    K = NK // N if N > 0 else 1
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: K = offset_gradient_accum.shape[0] / N must be in [1, {MAX_K}] (got {K})")
    if N * 3 * K >= 2 ** 31:
        raise ValueError(f"{who}: N * 3 K must be below 2^31 (got N = {N})")
    if offset_denom.dim() not in (1, 2) or offset_denom.shape[0] != NK or offset_denom.numel() != NK:
        raise ValueError(f"{who}: offset_denom must be [{NK}, 1] (got {list(offset_denom.shape)})")
    if n > N:
        raise ValueError(f"{who}: idx holds {n} rows, more than the {N} anchors")
    if neural_opacity.numel() != n * K or neural_opacity.dim() not in (1, 2) or neural_opacity.shape[0] != n * K:
        raise ValueError(f"{who}: neural_opacity must be [{n * K}, 1] (got {list(neural_opacity.shape)})")
    if tuple(offset_selection_mask.shape) != (n * K,):
        raise ValueError(f"{who}: offset_selection_mask must be [{n * K}] (got {list(offset_selection_mask.shape)})")
    if radii.dim() != 1:
        raise ValueError(f"{who}: radii must be [M] (got {list(radii.shape)})")
    M = radii.shape[0]
    if tuple(viewspace_grad.shape) != (M, 3):
        raise ValueError(f"{who}: viewspace_grad must be [{M}, 3] (got {list(viewspace_grad.shape)})")
    if M >= 2 ** 31:
        raise ValueError(f"{who}: M must be below 2^31 (got {M})")
    for name, t, _ in tensors[:4]:
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} is updated in place and must be contiguous")
    _ops.check_on_gpu(who, tensors)
    _ops.check_same_device(who, tensors, tensors[0][1].device)
    if check:
        _check_idx(who, idx, N)
    if n == 0:
        return None
    dev = idx.device
    scratch = _ops.scratch(_capi.lib().bsr_anchor_accumulate_scratch_bytes(n, K), dev)
    idx, neural_opacity, selection = idx.contiguous(), neural_opacity.contiguous(), offset_selection_mask.contiguous()
    radii, grad = radii.contiguous(), viewspace_grad.contiguous()
    _capi.call("bsr_anchor_accumulate", N, n, K, M, ptr(idx), ptr(neural_opacity), ptr(selection), ptr(radii),
               int(radii.dtype == torch.bool), ptr(grad), ptr(opacity_accum), ptr(anchor_demon),
               ptr(offset_gradient_accum), ptr(offset_denom), ptr(scratch), _ops.stream(dev))
    return None
