"""Time the point-cloud reprojection (include/bloomscene_reproject.h, bloomscene_amd.reproject) on the workload of
BloomScene.generate_pcd (bloomscene.py:428-656, "BS"): the cloud is built the way the reference builds it, then warped
into the 50 training frames.

    python tools/bench_reproject.py [--size 512] [--repeats 7] [--warmup 2] [--scipy-poses 1]

The cloud: 512 x 512 synthetic depth frames (smooth, 1.5 .. 2.5 away) under the ten rotate360 poses (yaws of 36 degrees
in the order 0 1 9 2 8 3 7 4 6 5, no translation).  Pose 0 lifts every pixel (BS:470-472); every later pose warps the
cloud so far into its camera (BS:479-504) and lifts the pixels that 1 - mask selects (BS:545-551), as the reference
appends them.  The border depth compensation of BS:554-580 is left out, as in the product.
Timed: `warp_points` into the 50 training poses -- for each generation pose its five hemisphere poses (a yaw or a pitch of
5 degrees about the point at the frame's centre depth, and the pose itself; BS:601-621).  One pass over the 50 poses is
bracketed by two device events; `repeats` passes, the median and the spread (max - min) are reported, and the median
per call.  The cloud-building loop (9 warps + 10 lifts, with its one host read per lift) is timed the same way, by a
host clock around a device synchronise.  Where scipy imports, the reference's own lines for one frame -- griddata
linear of the colours (BS:637), of the depths (BS:640, computed and never used there), and the two filters (BS:645,
647) -- are timed on the host for the first `--scipy-poses` training poses on the same points.  Which pass dominates is
read from a kernel trace of this tool, in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/bench_reproject.py --repeats 1 --scipy-poses 0).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.reproject import lift_pixels, warp_points  # noqa: E402


def rotate360_poses():
    poses = []
    for k in (0, 1, 9, 2, 8, 3, 7, 4, 6, 5):
        a = np.deg2rad(36.0 * k)
        poses.append((np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), np.zeros(3)))
    return poses


def hemisphere_poses(d):
    """The five camera-to-camera poses about the point at depth d: yaw +5, pitch -5, none, pitch +5, yaw -5 degrees."""
    out = []
    for th, phi in ((5, 0), (0, -5), (0, 0), (0, 5), (-5, 0)):
        t, p = np.deg2rad(th), np.deg2rad(phi)
        Ry = np.array([[np.cos(t), 0, -np.sin(t)], [0, 1, 0], [np.sin(t), 0, np.cos(t)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
        out.append((Ry @ Rx, np.array([d * np.sin(t), d * np.sin(p), (d - d * np.cos(t)) + (d - d * np.cos(p))])))
    return out


def synthetic_frame(S, k, dev):
    """Depth [S, S] float32 in 1.5 .. 2.5 and an image [S, S, 3] uint8, both smooth, different for every pose k."""
    y, x = torch.meshgrid(torch.linspace(0, 1, S, device=dev), torch.linspace(0, 1, S, device=dev), indexing="ij")
    depth = 2.0 + 0.3 * torch.sin(4.0 * x + k) * torch.cos(3.0 * y - 0.5 * k) + 0.2 * torch.cos(7.0 * (x + y) + k)
    image = torch.stack([0.5 + 0.5 * torch.sin(9 * x + k), 0.5 + 0.5 * torch.cos(8 * y - k), 0.5 + 0.5 * torch.sin(6 * (x - y))], dim=-1)
    return depth.float().contiguous(), (image * 255).round().to(torch.uint8).contiguous()


def build_cloud(S, K, poses, dev):
    """-> points [3, P], colors [P, 3], the centre depths, the points each pose added."""
    centre, added = [], []
    pts, col = None, None
    for k, (R, T) in enumerate(poses):
        depth, image = synthetic_frame(S, k, dev)
        centre.append(float(depth[S // 2 - 10:S // 2 + 10, S // 2 - 10:S // 2 + 10].mean()))
        if k == 0:
            p, c = lift_pixels(depth, image, K, R, T)
        else:
            w = warp_points(pts, col, K, R, T, S, S)
            p, c = lift_pixels(depth, image, K, R, T, select=w.mask == 0)
        added.append(p.shape[0])
        pts = p.T.contiguous() if pts is None else torch.cat([pts, p.T], dim=1)   # the reference keeps [3, P]
        col = c if col is None else torch.cat([col, c], dim=0)
    return pts, col, centre, added


def scipy_frame(points, colors, K, R, T, S):
    """The host work of one training frame of the reference (BS:621-648) with the scipy calls it makes -- two linear
    griddata interpolations onto the pixel grid and a 9 x 9 maximum / 11 x 11 minimum filter pair -- on the same points;
    -> seconds of each part."""
    from scipy.interpolate import griddata
    from scipy.ndimage import maximum_filter, minimum_filter
    t0 = time.perf_counter()
    p = K @ (R @ points + T.reshape(3, 1))
    with np.errstate(all="ignore"):
        u, v, z = p[0] / p[2], p[1] / p[2], p[2]
        valid = np.nonzero((z > 0) & (u >= 0) & (u <= S - 1) & (v >= 0) & (v <= S - 1))[0]
    uv = np.stack([u[valid], v[valid]], axis=1)
    pixels = np.stack(np.meshgrid(np.arange(S), np.arange(S)), axis=-1).reshape(-1, 2).astype(np.float32)
    t1 = time.perf_counter()
    griddata(uv, colors[valid], pixels, method="linear", fill_value=0)
    t2 = time.perf_counter()
    griddata(uv, z[valid], pixels, method="linear", fill_value=0)
    t3 = time.perf_counter()
    hit = np.zeros((S, S), dtype=np.uint8)
    hit[np.rint(uv[:, 1]).astype(np.int64), np.rint(uv[:, 0]).astype(np.int64)] = 1
    minimum_filter(maximum_filter(hit, size=9), size=11)
    t4 = time.perf_counter()
    return {"valid_points": int(len(valid)), "project_s": t1 - t0, "griddata_image_s": t2 - t1, "griddata_depth_s": t3 - t2,
            "filters_s": t4 - t3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-poses", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_reproject.py needs the GPU: there is no CPU path"
    dev = torch.device("cuda:0")
    S = args.size
    K = np.array([[5.8269e2 * S / 512, 0, S / 2], [0, 5.8269e2 * S / 512, S / 2], [0, 0, 1]], dtype=np.float64)
    gen = rotate360_poses()

    build_s = []
    for _ in range(1 + min(args.repeats, 3)):        # (the first pass is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pts, col, centre, added = build_cloud(S, K, gen, dev)
        torch.cuda.synchronize()
        build_s.append(time.perf_counter() - t0)
    build_s = build_s[1:]

    train = []
    for (Rw2i, Tw2i), d in zip(gen, centre):
        for Ri2j, Ti2j in hemisphere_poses(d):
            train.append((Ri2j @ Rw2i, Ri2j @ Tw2i + Ti2j))

    def one_pass():
        return [warp_points(pts, col, K, R, T, S, S) for R, T in train]

    for _ in range(args.warmup):
        out = one_pass()
    torch.cuda.synchronize()
    valid = [int((w.pixel >= 0).sum()) for w in out]
    covered = [float(w.mask.float().mean()) for w in out]
    again = one_pass()
    identical = all(torch.equal(a.image, b.image) and torch.equal(a.depth, b.depth) and torch.equal(a.mask, b.mask)
                    for a, b in zip(out, again))
    del out, again
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        one_pass()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()

    result = {
        "bench": "reproject", "size": S, "points": int(pts.shape[1]), "points_added_per_pose": added,
        "training_poses": len(train), "valid_points_min_median_max": [min(valid), int(np.median(valid)), max(valid)],
        "mask_coverage_median": float(np.median(covered)), "bit_identical_between_passes": identical,
        "warp_50_poses_ms_median": times[len(times) // 2], "warp_50_poses_ms_spread": times[-1] - times[0],
        "warp_ms_per_call_median": times[len(times) // 2] / len(train), "repeats": args.repeats,
        "build_cloud_s_median": float(np.median(build_s)), "build_cloud_s_spread": float(max(build_s) - min(build_s)),
    }
    if args.scipy_poses > 0:
        try:
            import scipy  # noqa: F401
        except ImportError:
            result["scipy"] = "not installed: the reference's lines were not timed"
        else:
            hp, hc = pts.cpu().numpy(), col.cpu().numpy()
            result["scipy_frames"] = [scipy_frame(hp, hc, K, R, T, S) for R, T in train[:args.scipy_poses]]
            result["scipy_note"] = "host time of one process on the GPU box's CPU, one run per frame"
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
