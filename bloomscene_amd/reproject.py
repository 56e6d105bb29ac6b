"""The point-cloud reprojection of BloomScene's scene-lifting stage on the MI355X (``BloomScene.generate_pcd``,
``bloomscene.py:428-656``, "BS"), in HIP behind ``include/bloomscene_reproject.h``.

    image, depth, mask, mask_hf, pixel = warp_points(points, colors, K, R, T, H, W, z_tolerance=0.05)   # BS:479-504, BS:621-648
    points, colors = lift_pixels(depth, image, K, R, T, select=None)                                    # BS:470-472, BS:545-551

``warp_points`` is NOT ``scipy.interpolate.griddata``: it is the deterministic function the header writes out (a bilinear
splat behind a soft z-buffer, resolved per pixel, with a 9 x 9 fill); the hit mask, the two mask filters, ``mask_hf``, the
validity rule and the rounded coordinates are the reference's exactly.  ``z_tolerance=None`` drops the visibility test, which
the reference does not have; 0.05 is a choice, not a tuned value.  Both run on the current torch stream and take their
scratch from torch's allocator; ``warp_points`` and ``lift_pixels(select=None)`` read nothing on the host (capturable into
a CUDA graph), ``lift_pixels`` with a selection reads one count.  Bit-identical from run to run.  No gradient; no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _capi
from . import _operands as _ops


class WarpResult(NamedTuple):
    image: torch.Tensor     # [H, W, 3] float32, 0 where mask is 0
    depth: torch.Tensor     # [H, W] float32, not masked
    mask: torch.Tensor      # [H, W] uint8: BS:498's mask2 / maskj
    mask_hf: torch.Tensor   # [H, W] uint8: BS:501-503
    pixel: torch.Tensor     # [P] int32: rint(v) * W + rint(u) of a valid point, -1 of an invalid one


def _host_array(who, name, a):
    """Step 1 for a camera operand: a host array-like -> float64 numpy."""
    if isinstance(a, torch.Tensor):
        if a.device.type != "cpu":
            raise TypeError(f"{who}: {name} must be a host array (got a tensor on {a.device})")
        a = a.detach().numpy()
    try:
        return np.asarray(a, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise TypeError(f"{who}: {name} must be a host array of numbers ({e})") from None


def _camera(who, first, second, T):
    """Step 3 for the camera: shapes, then the 21 doubles a native call takes."""
    for name, a, n in (first + (9,), second + (9,), ("T", T, 3)):
        if a.size != n or (n == 9 and a.shape != (3, 3)):
            raise ValueError(f"{who}: {name} must be {'3 x 3' if n == 9 else '3 values'} (got {list(a.shape)})")
    return (C.c_double * 21)(*first[1].reshape(-1), *second[1].reshape(-1), *T.reshape(-1))


def warp_points(points, colors, K, R, T, H, W, z_tolerance=0.05) -> WarpResult:
    """Reproject a coloured point cloud into the camera ``(K, R, T)`` (``bsr_warp_points``; the header has the function).

    ``points`` float32 ``[P, 3]`` or ``[3, P]`` (the reference keeps ``[3, P]``; ``[3, 3]`` reads as ``[P, 3]``), read in
    place through its two strides; ``colors`` float32 ``[P, 3]``; ``K`` 3 x 3, ``R`` 3 x 3 and ``T`` (3 values)
    world-to-camera, host arrays; ``z_tolerance`` a finite number >= 0, or None for no visibility test.
    ``border_valid_idx`` of BS:504 is ``(mask_hf.view(-1)[pixel[pixel >= 0].long()] == 1).nonzero()``."""
    who = "warp_points"
    _ops.check_tensors(who, [("points", points), ("colors", colors)])
    K, R, T = _host_array(who, "K", K), _host_array(who, "R", R), _host_array(who, "T", T)
    if points.requires_grad or colors.requires_grad:
        raise NotImplementedError(f"{who}: no gradient is implemented (detach the operands)")
    if colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError(f"{who}: colors must be [P, 3] (got {list(colors.shape)})")
    P = colors.shape[0]
    if tuple(points.shape) == (P, 3):
        ps, cs = points.stride(0), points.stride(1)
    elif tuple(points.shape) == (3, P):
        ps, cs = points.stride(1), points.stride(0)
    else:
        raise ValueError(f"{who}: points must be [{P}, 3] or [3, {P}] (got {list(points.shape)})")
    camera = _camera(who, ("K", K), ("R", R), T)
    H, W = int(H), int(W)
    if H < 3 or W < 3 or H * W >= 2 ** 31:
        raise ValueError(f"{who}: need H, W >= 3 and H * W below 2^31 (got {H}, {W})")
    if P >= 2 ** 31:
        raise ValueError(f"{who}: need fewer than 2^31 points (got {P})")
    if z_tolerance is not None and not (0.0 <= float(z_tolerance) < float("inf")):
        raise ValueError(f"{who}: z_tolerance must be a finite number >= 0 or None (got {z_tolerance})")
    _ops.check_on_gpu(who, [("points", points), ("colors", colors)])
    dev = points.device
    _ops.check_same_device(who, [("colors", colors)], dev)
    colors = colors.contiguous()
    image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    mask_hf = torch.empty(H, W, dtype=torch.uint8, device=dev)
    pixel = torch.empty(P, dtype=torch.int32, device=dev)
    scratch = _ops.scratch(_capi.lib().bsr_reproject_scratch_bytes(H, W), dev) if P else None
    _capi.call("bsr_warp_points", P, H, W, points.data_ptr(), ps, cs, colors.data_ptr(), camera,
               int(z_tolerance is not None), float(z_tolerance or 0.0), image.data_ptr(), depth.data_ptr(), mask.data_ptr(),
               mask_hf.data_ptr(), pixel.data_ptr(), _ops.ptr(scratch), _ops.stream(dev))
    return WarpResult(image, depth, mask, mask_hf, pixel)


def lift_pixels(depth, image, K, R, T, select=None):
    """Lift the pixels of a depth frame into the world (``bsr_lift_pixels``): BS:470-472 and BS:545-551.

    ``depth`` float32 ``[H, W]``; ``image`` float32 ``[H, W, 3]``, or uint8, which is divided by 255; ``K``, ``R``, ``T``
    as in ``warp_points`` (the two inverses are taken here, in float64); ``select`` bool or uint8 ``[H, W]`` or None for
    every pixel.  -> ``points [n, 3]``, ``colors [n, 3]`` float32 of the pixels where ``select`` is non-zero, in row-major
    order.  With a selection ``n`` is read on the host once."""
    who = "lift_pixels"
    named = [("depth", depth), ("image", image, (torch.float32, torch.uint8))]
    if select is not None:
        named.append(("select", select, (torch.bool, torch.uint8)))
    _ops.check_tensors(who, named, half_note=False)
    K, R, T = _host_array(who, "K", K), _host_array(who, "R", R), _host_array(who, "T", T)
    if depth.requires_grad or image.requires_grad:
        raise NotImplementedError(f"{who}: no gradient is implemented (detach the operands)")
    if depth.dim() != 2:
        raise ValueError(f"{who}: depth must be [H, W] (got {list(depth.shape)})")
    H, W = depth.shape
    if tuple(image.shape) != (H, W, 3):
        raise ValueError(f"{who}: image must be [{H}, {W}, 3] (got {list(image.shape)})")
    if select is not None and tuple(select.shape) != (H, W):
        raise ValueError(f"{who}: select must be [{H}, {W}] (got {list(select.shape)})")
    _camera(who, ("K", K), ("R", R), T)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{who}: need H, W >= 1 and H * W below 2^31 (got {H}, {W})")
    try:
        camera = _camera(who, ("K", np.linalg.inv(K)), ("R", np.linalg.inv(R)), T)
    except np.linalg.LinAlgError:
        raise ValueError(f"{who}: K and R must be invertible") from None
    named = [entry[:2] for entry in named]
    _ops.check_on_gpu(who, named)
    dev = depth.device
    _ops.check_same_device(who, named[1:], dev)
    depth, image = depth.contiguous(), image.contiguous()
    n, scratch = H * W, None
    if select is not None:
        select = select.contiguous().view(torch.uint8)
        scratch = _ops.scratch(_capi.lib().bsr_lift_scratch_bytes(H, W), dev)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        _capi.call("bsr_lift_count", H, W, select.data_ptr(), scratch.data_ptr(), total.data_ptr(), _ops.stream(dev))
        n = int(total.item())   # the one host read
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    colors = torch.empty(n, 3, dtype=torch.float32, device=dev)
    is_f = image.dtype == torch.float32
    _capi.call("bsr_lift_pixels", H, W, depth.data_ptr(), image.data_ptr() if is_f else None,
               None if is_f else image.data_ptr(), camera, _ops.ptr(select), _ops.ptr(scratch), n, points.data_ptr(),
               colors.data_ptr(), _ops.stream(dev))
    return points, colors
