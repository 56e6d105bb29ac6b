"""Time the voxel unique (include/bloomscene_voxelize.h) against what it replaces, at BloomScene's shapes.

    python tools/bench_voxelize.py [--iters 20] [--repeats 11] [--warmup 3] [--anchors 100000] [--points 2600000]
                                   [--fractions 0.01 0.05] [--host-repeats 3]

Anchor growing, GM:824-862 of GaussianModel.anchor_growing, 100 k anchors x 10 offsets, 50 features, per candidate
fraction and per cur_size level of GM:826 (voxel_size 0.001 x 16, 4, 1) -- three sides alternate in this process on the
same tensors:
    grow_level       bloomscene_amd.voxelize.grow_level: composite + quantise + unique in one native call
    grow_candidates  GM:824 in eager torch, then bloomscene_amd.densify.grow_candidates (eager quantise, gather, torch.unique)
    eager            GM:824-862 as written, torch.Tensor.scatter_reduce("amax") standing in for torch_scatter.scatter_max
Anchor creation, GM:435-438 at `points` float64 points and voxel_size 0.001:
    voxelize         bloomscene_amd.voxelize.voxelize on the device tensor
    torch_unique     torch.unique(torch.round(x / s), dim=0) * s on the device
    voxelize_sample  the drop-in on the numpy array: upload, voxelize, download
    numpy            GM:437 on the host -- seconds per call, so it is timed `host-repeats` times, one call each, apart
A figure is the time of `iters` back-to-back calls divided by `iters`, taken `repeats` times: the median, the spread
(max - min), and beside them the host's time in a call (the wall time of the same loop before the wait).  Results are
compared before anything is timed.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
from functools import reduce

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.densify import grow_candidates  # noqa: E402
from bloomscene_amd.voxelize import grow_level, voxelize, voxelize_sample  # noqa: E402

VOXEL_SIZE, SIZE_FACTORS = 0.001, (16, 4, 1)   # arguments.py:9-12 -> GM:826-827


def make_scene(N, K, F, seed):
    """Anchors on a noisy height field voxelised at VOXEL_SIZE (what create_from_pcd leaves), offsets of a few voxels in
    units of a per-anchor scaling, features."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xy = torch.rand(N, 2, device="cuda", generator=g) * 0.6
    z = 0.1 * torch.sin(9.0 * xy[:, :1]) * torch.cos(7.0 * xy[:, 1:]) + 0.002 * torch.randn(N, 1, device="cuda", generator=g)
    anchor = torch.round(torch.cat([xy, z], 1) / VOXEL_SIZE) * VOXEL_SIZE
    scaling = torch.rand(N, 6, device="cuda", generator=g) * 0.01 + 0.002           # get_scaling's [N, 6]
    offset = torch.randn(N, K, 3, device="cuda", generator=g)
    feat = torch.randn(N, F, device="cuda", generator=g)
    return anchor, offset, scaling, feat


def make_cloud(P, seed):
    """A float64 cloud on the host as create_from_pcd generates it: a surface sampled twice, the second time a fraction
    of a voxel away, so that about half the points share a voxel with another."""
    rng = np.random.default_rng(seed)
    twice = P - P // 2
    xy = rng.random((twice, 2)) * 1.2
    z = 0.1 * np.sin(9.0 * xy[:, :1]) * np.cos(7.0 * xy[:, 1:]) + 0.002 * rng.standard_normal((twice, 1))
    base = np.concatenate([xy, z], 1)
    return np.concatenate([base[:P // 2], base + rng.standard_normal((twice, 3)) * 0.0003], 0)


@torch.no_grad()
def all_xyz_of(anchor, offset, scaling):
    return anchor.unsqueeze(dim=1) + offset * scaling[:, :3].unsqueeze(dim=1)        # GM:824


@torch.no_grad()
def eager_grow(anchor, offset, scaling, candidate_mask, anchor_feat, cur_size):
    """GM:824-862, names as there."""
    n_offsets, feat_dim = offset.shape[1], anchor_feat.shape[1]
    all_xyz = all_xyz_of(anchor, offset, scaling)
    grid_coords = torch.round(anchor / cur_size).int()
    selected_xyz = all_xyz.view([-1, 3])[candidate_mask]
    selected_grid_coords = torch.round(selected_xyz / cur_size).int()
    selected_grid_coords_unique, inverse_indices = torch.unique(selected_grid_coords, return_inverse=True, dim=0)
    chunk_size = 4096
    max_iters = grid_coords.shape[0] // chunk_size + (1 if grid_coords.shape[0] % chunk_size != 0 else 0)
    remove_duplicates_list = []
    for i in range(max_iters):
        cur_remove_duplicates = (selected_grid_coords_unique.unsqueeze(1) ==
                                 grid_coords[i * chunk_size:(i + 1) * chunk_size, :]).all(-1).any(-1).view(-1)
        remove_duplicates_list.append(cur_remove_duplicates)
    remove_duplicates = reduce(torch.logical_or, remove_duplicates_list)
    remove_duplicates = ~remove_duplicates
    candidate_anchor = selected_grid_coords_unique[remove_duplicates] * cur_size
    new_feat = anchor_feat.unsqueeze(dim=1).repeat([1, n_offsets, 1]).view([-1, feat_dim])[candidate_mask]
    index = inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1))
    out = torch.zeros(selected_grid_coords_unique.shape[0], feat_dim, device=new_feat.device)
    new_feat = out.scatter_reduce(0, index, new_feat, "amax", include_self=False)[remove_duplicates]
    return candidate_anchor, new_feat


def time_alternating(fns, iters, repeats, warmup):
    """Per callable: {gpu_ms, spread_ms, host_ms} of one call, the callables taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times, host = [[] for _ in fns], [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            host[k].append((time.perf_counter() - t0) * 1e3 / iters)    # the host's share: calls may return before the GPU is done
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    return [{"gpu_ms": round(float(np.median(t)), 4), "spread_ms": round(float(max(t) - min(t)), 4),
             "host_ms": round(float(np.median(h)), 4)} for t, h in zip(times, host)]


def same(a, b):
    return bool(a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--anchors", type=int, default=100_000)
    ap.add_argument("--points", type=int, default=2_600_000)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.01, 0.05])
    ap.add_argument("--host-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxelize needs the GPU: there is no CPU path and no timing without one")
    N, K, F = args.anchors, 10, 50
    anchor, offset, scaling, feat = make_scene(N, K, F, seed=0)
    result = {"metric": "voxelize_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters,
              "repeats": args.repeats, "warmup": args.warmup, "anchors": N, "offsets": K, "features": F, "grow": [],
              "create": {}}
    g = torch.Generator(device="cuda").manual_seed(1)
    for fraction in args.fractions:
        mask = torch.rand(N * K, device="cuda", generator=g) < fraction
        for factor in SIZE_FACTORS:
            cur_size = VOXEL_SIZE * factor
            sides = [lambda: grow_level(anchor, offset, scaling, mask, feat, cur_size),
                     lambda: grow_candidates(anchor, all_xyz_of(anchor, offset, scaling), mask, feat, cur_size),
                     lambda: eager_grow(anchor, offset, scaling, mask, feat, cur_size)]
            got = [fn() for fn in sides]
            timed = time_alternating(sides, args.iters, args.repeats, args.warmup)
            result["grow"].append({"fraction": fraction, "cur_size": cur_size, "candidates": int(mask.sum()),
                                   "new_anchors": int(got[0][0].shape[0]),
                                   "same_as_grow_candidates": same(got[0], got[1]), "same_as_eager": same(got[0], got[2]),
                                   "grow_level": timed[0], "grow_candidates": timed[1], "eager": timed[2],
                                   "grow_candidates_over_grow_level": round(timed[1]["gpu_ms"] / timed[0]["gpu_ms"], 2),
                                   "eager_over_grow_level": round(timed[2]["gpu_ms"] / timed[0]["gpu_ms"], 2)})
    # anchor creation
    cloud = make_cloud(args.points, seed=2)
    on_device = torch.from_numpy(cloud).cuda()
    s = VOXEL_SIZE

    @torch.no_grad()
    def torch_unique():
        return torch.unique(torch.round(on_device / s), dim=0) * s

    sides = [lambda: voxelize(on_device, s), torch_unique, lambda: voxelize_sample(cloud, s)]
    timed = time_alternating(sides, args.iters, args.repeats, args.warmup)
    host_s = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        want = np.unique(np.round(cloud / s), axis=0) * s                              # GM:437
        host_s.append(time.perf_counter() - t0)
    got = voxelize_sample(cloud, s)
    dev = torch_unique()
    result["create"] = {"points": args.points, "dtype": "float64", "voxel_size": s, "voxels": int(got.shape[0]),
                        "same_as_numpy": bool(got.shape == want.shape and (got == want).all()),
                        "torch_unique_voxels": int(dev.shape[0]),   # (torch's GPU kernel divides by the reciprocal)
                        "voxelize": timed[0], "torch_unique": timed[1], "voxelize_sample": timed[2],
                        "numpy_host_ms": round(float(np.median(host_s)) * 1e3, 1), "numpy_repeats": args.host_repeats,
                        "torch_unique_over_voxelize": round(timed[1]["gpu_ms"] / timed[0]["gpu_ms"], 2),
                        "numpy_over_voxelize_sample": round(float(np.median(host_s)) * 1e3 / timed[2]["gpu_ms"], 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
