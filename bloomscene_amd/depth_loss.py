"""The depth-prior regularisation of BloomScene's loss on the MI355X: the min/max normalisations of
``bloomscene.py:298-305`` and ``HuberL1``, ``CMD`` and ``bilateral_filter`` of ``utils/loss.py:26-80,170-202`` as
``bloomscene.py:307-325`` calls them, in HIP behind ``include/bloomscene_depth_loss.h``.

    loss_depth = depth_prior_loss(render_pkg["depth"], original_depth, gt_image.permute(2, 1, 0),
                                  value=dep_value_lbd, domin=dep_domin_lbd, smooth=dep_smooth_lbd)      # bloomscene.py:298-325
    loss_depth, (lv, ld, ls) = depth_prior_loss(..., return_terms=True)
    r, o, h, b = depth_prior_maps(render_depth, prior_depth, rgb)                # the per-pixel maps, for measurement

The function, its gradient and the order of operations are written out in the header.  At most three kernels forward --
they leave a 128-byte stats block -- and two backward; every pixel sum is fixed-order fp64, so the four scalars and the
gradient are bit-identical from run to run.  The gradient goes to the rendered depth only: a prior or an image that
requires grad is refused, never given a silent zero.  ``rgb`` is read in place through its strides (the reference's
transposed ``permute(2, 1, 0)`` view costs no copy).  Everything runs on the current torch stream without a host
synchronisation (capturable into a CUDA graph) and takes its memory from torch's allocator.  There is no CPU path.

The terms reach the Gaussians only through a rasterizer built with ``depth_gradient=True``.
"""
from __future__ import annotations

import torch

from . import _capi
from . import _operands as _ops

VALUE, DOMIN, SMOOTH = 1, 2, 4      # BSR_DEPTH_PRIOR_VALUE, _DOMIN, _SMOOTH
STATS_BYTES = 128                   # BSR_DEPTH_PRIOR_STATS_BYTES
TRESH = 0.2                         # the constants the kernels implement
N_MOMENTS = 5
SPATIAL_SIGMA, COLOR_SIGMA, KERNEL_SIZE = 2.0, 5.0, 5


def _check(who, depth, prior, rgb, terms):
    """``_operands``' order of complaints.  ``prior`` / ``rgb`` may be None where the call has none.  -> (H, W)"""
    tensors = [(n, t) for n, t in (("render_depth", depth), ("prior_depth", prior), ("rgb", rgb)) if t is not None]
    _ops.check_tensors(who, tensors)
    for name, t in tensors[1:]:
        if t.requires_grad:
            raise NotImplementedError(f"{who}: the gradient to {name} is not implemented (detach it)")
    if depth.dim() == 3 and depth.shape[0] != 1:
        raise NotImplementedError(f"{who}: only a batch of one is implemented (got {list(depth.shape)})")
    if rgb is not None and rgb.dim() == 4 and rgb.shape[0] != 1:
        raise NotImplementedError(f"{who}: only a batch of one is implemented (got rgb {list(rgb.shape)})")
    if depth.dim() not in (2, 3):
        raise ValueError(f"{who}: render_depth must be [H, W] or [1, H, W] (got {list(depth.shape)})")
    H, W = depth.shape[-2:]
    if prior is not None and (prior.dim() not in (2, 3) or tuple(prior.shape[-2:]) != (H, W)
                              or (prior.dim() == 3 and prior.shape[0] != 1)):
        raise ValueError(f"{who}: prior_depth must be [H, W] or [1, H, W] like render_depth (got {list(prior.shape)} for "
                         f"{list(depth.shape)})")
    if rgb is not None and (rgb.dim() not in (3, 4) or tuple(rgb.shape[-3:]) != (H, W, 3)):
        raise ValueError(f"{who}: rgb must be [H, W, 3] or [1, H, W, 3] for a depth of {[H, W]} (got {list(rgb.shape)})")
    if H < 1 or W < 1:
        raise ValueError(f"{who}: H and W must be at least 1 (got {[H, W]})")
    if terms & VALUE and (H < 2 or W < 2):
        raise ValueError(f"{who}: the value term needs H and W of at least 2 (got {[H, W]})")
    if H * W >= 2 ** 31:
        raise ValueError(f"{who}: need fewer than 2^31 pixels (got {H * W})")
    _ops.check_on_gpu(who, tensors)
    for name, t in tensors[1:]:
        if t.device != depth.device:
            raise ValueError(f"{who}: {name} must be on {depth.device} (got {t.device})")
    return H, W


def _weights(who, value, domin, smooth):
    terms, w = 0, []
    for bit, name, v in ((VALUE, "value", value), (DOMIN, "domin", domin), (SMOOTH, "smooth", smooth)):
        if v is not None:
            if isinstance(v, torch.Tensor):
                raise TypeError(f"{who}: the weight {name} must be a number or None (a tensor would be a host wait)")
            terms |= bit
        w.append(0.0 if v is None else float(v))
    return terms, w


def _rgb_args(rgb):
    """-> (pointer, three element strides) of an [H, W, 3] / [1, H, W, 3] view, read in place"""
    if rgb is None:
        return None, 0, 0, 0
    sy, sx, sc = rgb.stride()[-3:]
    return rgb.data_ptr(), sy, sx, sc


class _DepthPrior(torch.autograd.Function):
    """inputs: the rendered depth [H, W] (dense), the prior (dense), rgb (any strides) or None, then the term mask, the
    three weights, ``normalise`` and whether to keep the stats.  outputs: the four 0-dim entries of out; only the first
    carries a gradient."""

    @staticmethod
    def forward(ctx, depth, prior, rgb, terms, w, normalise, keep):
        H, W = depth.shape
        dev = depth.device
        out = torch.empty(4, dtype=torch.float32, device=dev)
        stats = torch.empty(STATS_BYTES // 8, dtype=torch.float64, device=dev)
        scratch = _ops.scratch(_capi.lib().bsr_depth_prior_scratch_bytes(H, W), dev)
        _capi.call("bsr_depth_prior_forward", H, W, depth.data_ptr(), prior.data_ptr(), *_rgb_args(rgb), terms, w[0],
                   w[1], w[2], int(normalise), None, out.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                   _ops.stream(dev))
        if keep:
            ctx.save_for_backward(depth, prior, rgb, stats)
        ctx.call = (terms, w, normalise, keep)
        ctx.set_materialize_grads(False)
        parts = out.unbind(0)
        ctx.mark_non_differentiable(*parts[1:])
        return parts

    @staticmethod
    def backward(ctx, *gs):
        terms, w, normalise, keep = ctx.call
        if not keep:
            raise RuntimeError("depth_prior_loss: backward of a forward that kept no stats")
        g = gs[0]
        if g is None:
            return (None,) * 7
        depth, prior, rgb, stats = ctx.saved_tensors
        H, W = depth.shape
        dev = depth.device
        g = _ops.as_f32_contiguous(g)
        grad = torch.empty_like(depth)
        scratch = _ops.scratch(_capi.lib().bsr_depth_prior_scratch_bytes(H, W), dev)
        _capi.call("bsr_depth_prior_backward", H, W, depth.data_ptr(), prior.data_ptr(), *_rgb_args(rgb), terms, w[0],
                   w[1], w[2], int(normalise), stats.data_ptr(), g.data_ptr(), grad.data_ptr(), scratch.data_ptr(),
                   _ops.stream(dev))
        return (grad,) + (None,) * 6


def _plane(t):
    """[H, W] or [1, H, W] -> dense [H, W]"""
    return (t[0] if t.dim() == 3 else t).contiguous()


def _image(rgb):
    return None if rgb is None else (rgb[0] if rgb.dim() == 4 else rgb)


def _apply(depth, prior, rgb, terms, w, normalise):
    keep = torch.is_grad_enabled() and depth.requires_grad
    return _DepthPrior.apply(_plane(depth), _plane(prior), _image(rgb) if terms & VALUE else None, terms, tuple(w),
                             bool(normalise), keep)


def depth_prior_loss(render_depth, prior_depth, rgb, value=None, domin=None, smooth=None, normalise=True,
                     return_terms=False):
    """``value * HuberL1 + domin * CMD + smooth * bilateral_filter`` of bloomscene.py:298-325 on the (``normalise``:
    min/max-normalised) depths.  ``render_depth``, ``prior_depth`` float32 ``[H, W]`` or ``[1, H, W]`` on the GPU; ``rgb``
    float32 ``[H, W, 3]`` or ``[1, H, W, 3]`` with any strides (needed by the value term only; may be None without it).
    A weight of None switches its term off.  -> the 0-dim loss, one autograd node, differentiable in ``render_depth``; with
    ``return_terms`` also ``(value, domin, smooth)``, three detached 0-dim tensors (unweighted; 0 for a term that is
    off)."""
    who = "depth_prior_loss"
    terms, w = _weights(who, value, domin, smooth)
    _check(who, render_depth, prior_depth, rgb, terms)
    if terms & VALUE and rgb is None:
        raise ValueError(f"{who}: the value term needs rgb")
    loss, lv, ld, ls = _apply(render_depth, prior_depth, rgb, terms, w, normalise)
    return (loss, (lv, ld, ls)) if return_terms else loss


@torch.no_grad()
def depth_prior_maps(render_depth, prior_depth, rgb, normalise=True):
    """``(r, o, h, b)`` of the header, float32 ``[H, W]``: the two normalised depths, the HuberL1 map and the bilateral
    map (for measurement: no gradient)."""
    who = "depth_prior_maps"
    H, W = _check(who, render_depth, prior_depth, rgb, VALUE | SMOOTH)
    d, p, img = _plane(render_depth), _plane(prior_depth), _image(rgb)
    dev = d.device
    nbytes, stream, rgb_args = _capi.lib().bsr_depth_prior_scratch_bytes(H, W), _ops.stream(dev), _rgb_args(img)

    def run(first, second, terms):
        out = torch.empty(4, dtype=torch.float32, device=dev)
        maps = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        stats = torch.empty(STATS_BYTES // 8, dtype=torch.float64, device=dev)
        scratch = _ops.scratch(nbytes, dev)
        _capi.call("bsr_depth_prior_forward", H, W, first.data_ptr(), second.data_ptr(), *rgb_args, terms, 1.0, 1.0,
                   1.0, int(bool(normalise)), maps.data_ptr(), out.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
                   stream)
        return maps

    m = run(d, p, VALUE | SMOOTH)
    o = run(p, p, 0)[0]          # (r of the prior itself)
    return m[0], o, m[1], m[2]


class HuberL1:
    """``HuberL1`` of utils/loss.py:170-202 (same signature): ``HuberL1(tresh=0.2)(pred, gt, rgb)`` -> the 0-dim
    "scalar" loss, differentiable in ``pred``.  ``pred`` / ``gt`` hold H * W elements for ``rgb`` ``[..., H, W, 3]`` (the
    reference reshapes to 512 x 512; here to the image's own H, W).  Only ``tresh = 0.2`` and "scalar"."""

    def __init__(self, tresh=TRESH, implementation="scalar", **kwargs):
        if tresh != TRESH:
            raise NotImplementedError(f"HuberL1: only tresh = {TRESH} is implemented (got tresh = {tresh})")
        if implementation != "scalar":
            raise NotImplementedError(f'HuberL1: only implementation = "scalar" is implemented (got implementation = '
                                      f'{implementation!r})')
        self.tresh = tresh
        self.implementation = implementation

    def forward(self, pred, gt, rgb):
        who = "HuberL1"
        _ops.check_tensors(who, [("pred", pred), ("gt", gt), ("rgb", rgb)])
        if rgb.dim() not in (3, 4) or rgb.shape[-1] != 3:
            raise ValueError(f"{who}: rgb must be [H, W, 3] or [1, H, W, 3] (got {list(rgb.shape)})")
        H, W = rgb.shape[-3:-1]
        if pred.numel() != H * W or gt.numel() != H * W:
            raise ValueError(f"{who}: pred and gt must hold H * W = {H * W} elements (got {list(pred.shape)} and "
                             f"{list(gt.shape)})")
        pred, gt = pred.reshape(H, W), gt.reshape(H, W)
        _check(who, pred, gt, rgb, VALUE)
        return _apply(pred, gt, rgb, VALUE, (1.0, 0.0, 0.0), False)[0]

    __call__ = forward


class CMD:
    """``CMD`` of utils/loss.py:26-60 (same signature) for a batch of one: ``CMD()(x1, x2, n_moments=5)`` -> 0-dim,
    differentiable in ``x1``.  ``x1`` ``[1, H, W]``, ``x2`` ``[1, H, W]`` or ``[1, 1, H, W]``.  Only ``n_moments = 5``."""

    def forward(self, x1, x2, n_moments=N_MOMENTS):
        who = "CMD"
        _ops.check_tensors(who, [("x1", x1), ("x2", x2)])
        if n_moments != N_MOMENTS:
            raise NotImplementedError(f"{who}: only n_moments = {N_MOMENTS} is implemented (got n_moments = {n_moments})")
        if x1.dim() >= 1 and x1.shape[0] != 1 and x1.dim() != 2:
            raise NotImplementedError(f"{who}: only a batch of one is implemented (got x1 {list(x1.shape)})")
        if x2.dim() == 4 and x2.shape[:2] == (1, 1):
            x2 = x2[0]
        _check(who, x1, x2, None, DOMIN)
        return _apply(x1, x2, None, DOMIN, (0.0, 1.0, 0.0), False)[0]

    __call__ = forward


def bilateral_filter(depth, spatial_sigma=SPATIAL_SIGMA, color_sigma=COLOR_SIGMA, kernel_size=KERNEL_SIZE):
    """``bilateral_filter`` of utils/loss.py:63-80 for ``depth`` ``[1, H, W]`` -> 0-dim, differentiable in ``depth``.
    Only the parameters BloomScene calls it with: ``spatial_sigma = 2``, ``color_sigma = 5`` (NOT the reference's own
    default of 0.1, hence the default here) and ``kernel_size = 5``."""
    who = "bilateral_filter"
    _ops.check_tensors(who, [("depth", depth)])
    for name, got, want in (("spatial_sigma", spatial_sigma, SPATIAL_SIGMA), ("color_sigma", color_sigma, COLOR_SIGMA),
                            ("kernel_size", kernel_size, KERNEL_SIZE)):
        if got != want:
            raise NotImplementedError(f"{who}: only {name} = {want} is implemented (got {name} = {got})")
    _check(who, depth, None, None, SMOOTH)
    return _apply(depth, depth.detach(), None, SMOOTH, (0.0, 0.0, 1.0), False)[0]
