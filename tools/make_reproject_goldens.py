#!/usr/bin/env python3
"""Write ``tests/golden/reproject/reproject_*.npz``: what scipy computes where ``BloomScene.generate_pcd`` (bloomscene.py:479-504,
621-648) calls it, on small synthetic scenes, as DATA for ``tests/test_reproject_cpu.py`` / ``test_reproject_gpu.py``.

This is our own code calling scipy (the build machine has it; the GPU tests never import it).  Each file holds
  inputs:   points [3, P] float32, colors [P, 3] float32, K, R, T float64, H, W
  scipy:    linear, nearest   griddata(method=...) of the colours on the pixel grid, [H, W, 3] float64, fill_value 0
            depth_linear      griddata linear of the depths
            known, mask       maximum_filter(size 9) of the hit mask, minimum_filter(size 11) of that
  numpy:    valid_idx, round_coord [2, n] (x then y), mask_hf
The poses are the hemisphere poses of the scene-lifting stage as data (a yaw or a pitch of 5 degrees about a point at the
centre depth) and one plain 15 degree yaw.  A case is refused if any projected coordinate lies within 1e-9 of a rounding
or validity boundary: BLAS may fuse multiply-adds where the product's kernels do not, and no recorded decision may hang on
that.

    python tools/make_reproject_goldens.py            # rewrites every file (deterministic: fixed seeds)
"""
import os
import sys

import numpy as np
from scipy.interpolate import griddata
from scipy.ndimage import maximum_filter, minimum_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reproject")


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])


def rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def hemisphere_pose(th, phi, d):
    """World-to-camera (R, T) of a camera turned by th about y and phi about x around the point at depth d."""
    s, c = np.sin(np.deg2rad(th)), np.cos(np.deg2rad(th))
    sp, cp = np.sin(np.deg2rad(phi)), np.cos(np.deg2rad(phi))
    return rot_y(th) @ rot_x(phi), np.array([d * s, d * sp, (d - d * c) + (d - d * cp)])


def yaw_pose(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), np.zeros(3)


def intrinsics(H, W):
    return np.array([[1.1 * W, 0, W / 2], [0, 1.1 * W, H / 2], [0, 0, 1]], dtype=np.float64)


def scene(kind, H, W, P, seed):
    """P points seen from the identity camera at uniformly random sub-pixel positions of the frame (and a margin around
    it, so that a turned camera still sees a covered frame edge), on a smooth surface with smooth colours; "two_layer"
    puts a disc of a nearer surface with its own colours in front."""
    rng = np.random.default_rng(seed)
    K = intrinsics(H, W)
    px = rng.uniform(-0.15 * W, 1.15 * W, P)
    py = rng.uniform(-0.15 * H, 1.15 * H, P)
    sx, sy = px / W, py / H
    depth = 2.0 + 0.25 * np.sin(2.1 * sx + 0.4) * np.cos(1.7 * sy - 0.2)
    col = np.stack([0.5 + 0.4 * np.sin(3.0 * sx + 1.0), 0.5 + 0.4 * np.cos(2.5 * sy + 0.3),
                    0.5 + 0.35 * np.sin(2.0 * (sx + sy))], axis=1)
    if kind == "two_layer":
        near = (sx - 0.45) ** 2 + (sy - 0.5) ** 2 < 0.2 ** 2
        depth = np.where(near, 1.2 + 0.05 * sx, depth)
        col = np.where(near[:, None], np.stack([0.9 - 0.3 * sx, 0.2 + 0.2 * sy, 0.1 + 0 * sx], axis=1), col)
    cam = np.linalg.inv(K) @ np.stack([px * depth, py * depth, depth])
    return cam.astype(np.float32), col.astype(np.float32), K, 2.0


def record(name, kind, H, W, P, seed, pose):
    points, colors, K, d = scene(kind, H, W, P, seed)
    R, T = pose(d)
    # the reference's lines, on numpy / BLAS / scipy
    cam = R.dot(points) + T.reshape(3, 1)
    pix = np.matmul(K, cam)
    u, v, z = pix[0] / pix[2], pix[1] / pix[2], pix[2]
    valid_idx = np.where(np.logical_and.reduce((z > 0, u >= 0, u <= W - 1, v >= 0, v <= H - 1)))[0]
    # no decision within 1e-9 of its boundary
    for a, hi in ((u, W - 1), (v, H - 1)):
        assert np.abs(a).min() > 1e-9 and np.abs(a - hi).min() > 1e-9, name
        inside = a[valid_idx]
        assert np.abs(inside - np.floor(inside) - 0.5).min() > 1e-9, name
    assert np.abs(z).min() > 1e-9, name
    coord = np.stack([u[valid_idx], v[valid_idx]])
    round_coord = np.round(coord).astype(np.int32)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    grid = np.stack((gx, gy), axis=-1).reshape(-1, 2)
    linear = griddata(coord.T, colors[valid_idx], grid, method="linear", fill_value=0).reshape(H, W, 3)
    nearest = griddata(coord.T, colors[valid_idx], grid, method="nearest").reshape(H, W, 3)
    depth_linear = griddata(coord.T, z[valid_idx], grid, method="linear", fill_value=0).reshape(H, W)
    hit = np.zeros((H, W), dtype=np.float32)
    hit[round_coord[1], round_coord[0]] = 1
    known = maximum_filter(hit, size=(9, 9), axes=(0, 1))
    mask = minimum_filter((known != 0) * 1, size=(11, 11), axes=(0, 1))
    # a pixel whose lower or right neighbour has another mask value; the last row and column repeat their neighbour's
    hf = (mask[:-1, :-1] != mask[1:, :-1]) | (mask[:-1, :-1] != mask[:-1, 1:])
    hf = np.pad(hf, ((0, 1), (0, 1)), "edge")
    path = os.path.join(OUT, f"reproject_{name}.npz")
    np.savez_compressed(path, points=points, colors=colors, K=K, R=R, T=T, H=H, W=W, kind=kind,
                        linear=linear, nearest=nearest, depth_linear=depth_linear, hit=hit.astype(np.uint8),
                        known=known.astype(np.uint8), mask=mask.astype(np.uint8), mask_hf=hf.astype(np.uint8),
                        valid_idx=valid_idx.astype(np.int64), round_coord=round_coord)
    print(f"{os.path.relpath(path, ROOT)}: {H}x{W}, P = {P}, {len(valid_idx)} valid, mask covers {int(mask.sum())} pixels, "
          f"{os.path.getsize(path)} bytes")


CASES = [
    # name, kind, H, W, P, seed, pose(centre depth)
    ("smooth_64x64_yaw_p5", "smooth", 64, 64, 3901, 1, lambda d: hemisphere_pose(5, 0, d)),
    ("smooth_64x64_pitch_m5", "smooth", 64, 64, 3901, 2, lambda d: hemisphere_pose(0, -5, d)),
    ("smooth_40x48_yaw_m5", "smooth", 40, 48, 2500, 3, lambda d: hemisphere_pose(-5, 0, d)),
    ("smooth_17x33_yaw15", "smooth", 17, 33, 700, 4, lambda d: yaw_pose(15)),
    ("two_layer_40x48_yaw_p5", "two_layer", 40, 48, 2500, 5, lambda d: hemisphere_pose(5, 0, d)),
    ("two_layer_17x33_pitch_p5", "two_layer", 17, 33, 700, 6, lambda d: hemisphere_pose(0, 5, d)),
]


def main():
    for case in CASES:
        record(*case)
    return 0


if __name__ == "__main__":
    sys.exit(main())
