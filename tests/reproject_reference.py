"""numpy restatement of ``include/bloomscene_reproject.h``: ``warp_points`` (the seven steps) and ``lift_pixels``.

Every output is the header's pure function evaluated in the header's order: fp64 sums k-ascending with no fused
multiply-add (numpy's element-wise ``*`` and ``+`` round each operation), 64-bit integer sums for the splat (exact in any
order), the fill row-major over its window.  The GPU tests compare bit for bit with this module; the CPU tests compare
this module with scipy's results recorded under ``tests/golden/reproject/reproject_*.npz``.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

SHIFT = 28                      # BSR_REPROJECT_SHIFT: the splat's fixed point
CLAMP = float(2 ** 62)          # step 4's clamp of a contribution's magnitude before it is rounded: 2^62
FILL_RADIUS = 4                 # the 9 x 9 window of steps 5 and 7
ERODE_RADIUS = 5                # the 11 x 11 window of step 7
RING = 2


class Warp(NamedTuple):
    image: np.ndarray     # [H, W, 3] float32
    depth: np.ndarray     # [H, W] float32
    mask: np.ndarray      # [H, W] uint8
    mask_hf: np.ndarray   # [H, W] uint8
    pixel: np.ndarray     # [P] int32
    # intermediate results, for the CPU tests
    hit: np.ndarray       # [H, W] uint8
    known: np.ndarray     # [H, W] uint8
    resolved: np.ndarray  # [H, W] bool


def _sum3(m, row, x):
    """(m[row, 0] * x[0] + m[row, 1] * x[1]) + m[row, 2] * x[2] in fp64, each operation rounded."""
    return (m[row, 0] * x[0] + m[row, 1] * x[1]) + m[row, 2] * x[2]


def project(points_3p, K, R, T):
    """Step 1's arithmetic: ``points_3p`` float32 ``[3, P]`` -> ``u, v, z`` float64 ``[P]``."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    x = np.asarray(points_3p, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        cam = [_sum3(R, i, x) + T[i] for i in range(3)]
        p = [_sum3(K, i, cam) for i in range(3)]
        return p[0] / p[2], p[1] / p[2], p[2]


def window_max(a, radius):
    """Maximum over the (2 radius + 1)^2 window clipped to the frame."""
    H, W = a.shape
    out = np.empty_like(a)
    for r in range(H):
        for c in range(W):
            out[r, c] = a[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1].max()
    return out


def window_min(a, radius):
    H, W = a.shape
    out = np.empty_like(a)
    for r in range(H):
        for c in range(W):
            out[r, c] = a[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1].min()
    return out


def warp_points(points, colors, K, R, T, H, W, z_tolerance=0.05) -> Warp:
    """``points`` float32 ``[P, 3]`` or ``[3, P]`` (``[3, 3]`` reads as ``[P, 3]``), ``colors`` float32 ``[P, 3]``."""
    points = np.asarray(points, np.float32)
    colors = np.asarray(colors, np.float32).reshape(-1, 3)
    P = colors.shape[0]
    pts = points.T if points.shape == (P, 3) else points
    assert pts.shape == (3, P) and H >= 3 and W >= 3
    HW = H * W
    one_tol = None if z_tolerance is None else 1.0 + float(z_tolerance)

    # 1. projection
    u, v, z = project(pts, K, R, T)
    with np.errstate(all="ignore"):
        valid = (z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & np.isfinite(colors).all(axis=1)
    idx = np.nonzero(valid)[0]
    u, v, z = u[idx], v[idx], z[idx]
    pixel = np.full(P, -1, np.int32)
    pixel[idx] = (np.rint(v).astype(np.int64) * W + np.rint(u).astype(np.int64)).astype(np.int32)
    with np.errstate(over="ignore"):
        zf = z.astype(np.float32)

    # 2. hit mask
    hit = np.zeros(HW, np.uint8)
    hit[pixel[idx]] = 1

    # 3. the footprint and the soft z-buffer
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = u - x0, v - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    corners = []   # (pixel index, weight, selector of the points that touch it)
    for dy, dx, w in ((0, 0, (1.0 - fx) * (1.0 - fy)), (0, 1, fx * (1.0 - fy)), (1, 0, (1.0 - fx) * fy), (1, 1, fx * fy)):
        ok = (w > 0) & (x0 + dx < W) & (y0 + dy < H)
        corners.append(((y0 + dy) * W + (x0 + dx), w, ok))
    zbits = np.full(HW, 0xFFFFFFFF, np.uint32)
    for q, w, ok in corners:
        np.minimum.at(zbits, q[ok], zf[ok].view(np.uint32))
    zmin = zbits.view(np.float32).astype(np.float64)   # (the all-ones pattern, a NaN, is never compared: no point is there)

    # 4. the fixed-point splat
    acc = np.zeros((5, HW), np.int64)
    chan = [np.ones(len(idx)), colors[idx, 0].astype(np.float64), colors[idx, 1].astype(np.float64),
            colors[idx, 2].astype(np.float64), zf.astype(np.float64)]
    for q, w, ok in corners:
        if one_tol is not None:
            with np.errstate(invalid="ignore"):
                ok = ok & (zf.astype(np.float64) <= zmin[np.where(ok, q, 0)] * one_tol)
        for k in range(5):
            with np.errstate(over="ignore"):
                t = np.clip(w[ok] * chan[k][ok] * float(2 ** SHIFT), -CLAMP, CLAMP)
            np.add.at(acc[k], q[ok], np.rint(t).astype(np.int64))
    resolved = acc[0] > 0
    val = np.zeros((HW, 4), np.float32)
    den = acc[0][resolved].astype(np.float64)
    for k in range(4):
        val[resolved, k] = (acc[k + 1][resolved].astype(np.float64) / den).astype(np.float32)
    val = val.reshape(H, W, 4)
    resolved = resolved.reshape(H, W)
    hit = hit.reshape(H, W)

    # 7 (first half). known, mask
    known = window_max(hit, FILL_RADIUS)
    mask = window_min(known, ERODE_RADIUS)

    # 5. fill
    for r, c in zip(*np.nonzero((known == 1) & ~resolved)):
        r0, r1, c0, c1 = max(r - FILL_RADIUS, 0), min(r + FILL_RADIUS, H - 1), max(c - FILL_RADIUS, 0), min(c + FILL_RADIUS, W - 1)
        res = resolved[r0:r1 + 1, c0:c1 + 1]
        if not res.any():
            continue   # (the header's argument says this does not happen; the value stays 0)
        d = val[r0:r1 + 1, c0:c1 + 1, 3]
        take = res.copy()
        if one_tol is not None:
            take &= d.astype(np.float64) <= one_tol * float(d[res].min())
        s = np.zeros(4, np.float64)
        sw = 0.0
        for rr in range(r0, r1 + 1):
            for cc in range(c0, c1 + 1):
                if take[rr - r0, cc - c0]:
                    wgt = 1.0 / float((rr - r) ** 2 + (cc - c) ** 2)
                    s = s + wgt * val[rr, cc].astype(np.float64)
                    sw = sw + wgt
        if sw > 0:
            val[r, c] = (s / sw).astype(np.float32)

    # 6. border ring (the clamp is the identity away from the outermost row and column)
    rs = np.clip(np.arange(H), 1, H - 2)
    cs = np.clip(np.arange(W), 1, W - 2)
    val = val[rs][:, cs]

    # 7. masks
    image = np.where(mask[..., None] == 1, val[..., :3], np.float32(0)).astype(np.float32)
    depth = np.ascontiguousarray(val[..., 3])
    m = mask.astype(np.int32)
    hf = np.abs(m[:H - 1, :W - 1] - m[1:, :W - 1]) + np.abs(m[:H - 1, :W - 1] - m[:H - 1, 1:])
    mask_hf = (np.pad(hf, ((0, 1), (0, 1)), "edge") >= 1).astype(np.uint8)
    return Warp(image, depth, mask, mask_hf, pixel, hit, known, resolved)


def lift_pixels(depth, image, K, R, T, select=None):
    """-> ``points [n, 3]`` float32, ``colors [n, 3]`` float32 of the selected pixels in row-major order."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    Kinv = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
    Rinv = np.linalg.inv(np.asarray(R, np.float64).reshape(3, 3))
    T = np.asarray(T, np.float64).reshape(3)
    sel = np.arange(H * W) if select is None else np.nonzero(np.asarray(select).reshape(-1) != 0)[0]
    r, c = sel // W, sel % W
    d = depth.reshape(-1)[sel]
    with np.errstate(all="ignore"):
        a = [(c.astype(np.float32) * d).astype(np.float64), (r.astype(np.float32) * d).astype(np.float64), d.astype(np.float64)]
        cam = [_sum3(Kinv, i, a) - T[i] for i in range(3)]
        world = np.stack([_sum3(Rinv, i, cam) for i in range(3)], axis=1).astype(np.float32)
    image = np.asarray(image)
    flat = image.reshape(-1, 3)[sel]
    colors = flat.astype(np.float32) / np.float32(255.0) if image.dtype == np.uint8 else flat.astype(np.float32)
    return world, colors
