"""The photometric term of BloomScene's loss on the MI355X: ``l1_loss`` and ``ssim`` of ``utils/loss.py:83-134`` and their
combination of ``bloomscene.py:284-287``, in HIP behind ``include/bloomscene_loss.h``.

    loss_rgb = photometric_loss(image, gt_image, lambda_dssim)                   # bloomscene.py:285-286
    loss_rgb, (Ll1, s) = photometric_loss(image, gt_image, lambda_dssim, return_terms=True)
    s = ssim(img1, img2)                                                         # utils/loss.py:103, differentiable in img1
    m = ssim_map(image, gt_image)                                                # the map itself, for measurement

The function, its gradient and the order of operations are written out in the header.  One kernel forward -- it leaves
three per-pixel partial derivatives -- and one kernel backward, which convolves them once more; both sums are fixed-order
fp64, so the three scalars are bit-identical from run to run.  The gradient goes to the FIRST image only: a second image
that requires grad is refused, never given a silent zero.  Everything runs on the current torch stream without a host
synchronisation (capturable into a CUDA graph) and takes its memory from torch's allocator.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _capi
from . import _operands as _ops

WINDOW_SIZE = 11     # the only window the kernels implement (gaussian(11, 1.5), the header's constants)


def _check(who, first, second, names):
    """``_operands``' order of complaints."""
    tensors = list(zip(names, (first, second)))
    _ops.check_tensors(who, tensors)
    if second.requires_grad:
        raise NotImplementedError(f"{who}: the gradient to {names[1]} is not implemented (detach it)")
    if first.dim() not in (3, 4):
        raise ValueError(f"{who}: {names[0]} must be [C, H, W] or [B, C, H, W] (got {list(first.shape)})")
    if first.shape != second.shape:
        raise ValueError(f"{who}: {names[0]} and {names[1]} must have one shape (got {list(first.shape)} and "
                         f"{list(second.shape)})")
    if first.shape[-1] < 1 or first.shape[-2] < 1:
        raise ValueError(f"{who}: H and W must be at least 1 (got {list(first.shape)})")
    if first.numel() >= 2 ** 31:
        raise ValueError(f"{who}: need fewer than 2^31 elements (got {first.numel()})")
    _ops.check_on_gpu(who, tensors)
    if first.device != second.device:
        raise ValueError(f"{who}: both images must be on {first.device} (got {second.device})")


def _shape(t):
    return tuple(t.shape) if t.dim() == 4 else (1,) + tuple(t.shape)


LOSS, L1, SSIM = 0, 1, 2     # positions of the header's out[3]


class _Photometric(torch.autograd.Function):
    """inputs: image, gt (dense), then lambda, which of out[3] is the differentiable output, whether to keep the partials.
    outputs: the three 0-dim entries of out; only ``which`` carries a gradient."""

    @staticmethod
    def forward(ctx, image, gt, lam, which, keep):
        B, C, H, W = shape = _shape(image)
        dev = image.device
        out = torch.empty(3, dtype=torch.float32, device=dev)
        partials = torch.empty((3,) + shape, dtype=torch.float32, device=dev) if keep else None
        scratch = _ops.scratch(_capi.lib().bsr_photometric_scratch_bytes(B, C, H, W), dev)
        _capi.call("bsr_photometric_forward", B, C, H, W, image.data_ptr(), gt.data_ptr(), lam, _ops.ptr(partials),
                   None, out.data_ptr(), scratch.data_ptr(), _ops.stream(dev))
        ctx.save_for_backward(image, gt, partials)
        ctx.call = (shape, lam, which)
        ctx.set_materialize_grads(False)     # (no zeros for the two outputs that carry no gradient)
        terms = out.unbind(0)
        ctx.mark_non_differentiable(*(t for k, t in enumerate(terms) if k != which))
        return terms

    @staticmethod
    def backward(ctx, *gs):
        image, gt, partials = ctx.saved_tensors
        (B, C, H, W), lam, which = ctx.call
        if partials is None:
            raise RuntimeError("photometric_loss: backward of a forward that kept no partials")
        g = gs[which]
        if g is None:
            return None, None, None, None, None
        # d S = -d loss at lambda = 1 (the header): the sign goes into the upstream scalar
        g = _ops.as_f32_contiguous(-g if which == SSIM else g)
        grad = torch.empty_like(image)
        _capi.call("bsr_photometric_backward", B, C, H, W, image.data_ptr(), gt.data_ptr(), partials.data_ptr(), lam,
                   g.data_ptr(), grad.data_ptr(), _ops.stream(image.device))
        return grad, None, None, None, None


def _apply(image, gt, lam, which):
    keep = torch.is_grad_enabled() and image.requires_grad
    return _Photometric.apply(image.contiguous(), gt.contiguous(), float(lam), which, keep)


@torch.no_grad()
def ssim_map(image, gt):
    """The SSIM map ``m`` of the header, float32 in the shape of ``image`` (for measurement: no gradient)."""
    _check("ssim_map", image, gt, ("image", "gt"))
    image, gt = image.contiguous(), gt.contiguous()
    B, C, H, W = _shape(image)
    out = torch.empty(3, dtype=torch.float32, device=image.device)
    m = torch.empty_like(image)
    scratch = _ops.scratch(_capi.lib().bsr_photometric_scratch_bytes(B, C, H, W), image.device)
    _capi.call("bsr_photometric_forward", B, C, H, W, image.data_ptr(), gt.data_ptr(), 1.0, None, m.data_ptr(),
               out.data_ptr(), scratch.data_ptr(), _ops.stream(image.device))
    return m


def photometric_loss(image, gt, lambda_dssim=0.2, return_terms=False):
    """``(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt))`` of bloomscene.py:285-286.
    ``image``, ``gt`` float32 ``[C, H, W]`` or ``[B, C, H, W]`` on the GPU (made contiguous if they are not); ``gt`` must
    not require grad.  -> the 0-dim loss, differentiable in ``image`` through one backward kernel; with ``return_terms``
    also ``(l1, ssim)``, two detached 0-dim tensors."""
    _check("photometric_loss", image, gt, ("image", "gt"))
    loss, l1, s = _apply(image, gt, lambda_dssim, LOSS)
    return (loss, (l1, s)) if return_terms else loss


def ssim(img1, img2, window_size=11, size_average=True):
    """``ssim`` of utils/loss.py:103-111 (same signature): the mean of the SSIM map, 0-dim, differentiable in ``img1``.
    The same two kernels with lambda = 1.  Only ``window_size = 11`` and ``size_average = True``."""
    _ops.check_tensors("ssim", [("img1", img1), ("img2", img2)])   # (dtypes before the NotImplementedErrors)
    if window_size != WINDOW_SIZE:
        raise NotImplementedError(f"ssim: only window_size = {WINDOW_SIZE} is implemented (got {window_size})")
    if not size_average:
        raise NotImplementedError("ssim: size_average = False is not implemented")
    _check("ssim", img1, img2, ("img1", "img2"))
    return _apply(img1, img2, 1.0, SSIM)[SSIM]
