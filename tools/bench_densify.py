"""Time grow_candidates (include/bloomscene_densify.h) against the eager lines it replaces, GM:829-862 of BloomScene's
GaussianModel.anchor_growing, at BloomScene's shape: 100 k anchors x 10 offsets, 50 features, a seeded 5 % candidate
mask, at the three cur_size levels of GM:826 (voxel_size 0.001 x 16, 4, 1).

    python tools/bench_densify.py [--steps 20] [--warmup 3] [--anchors 100000] [--no-atomics]

Both sides run in this process on the same tensors, alternating, each call timed with events after `warmup` calls of
both; the figure is the median over `steps`.  The eager side is GM:829-862 as written (the chunked all-pairs comparison,
the repeated [N * K, F] feature tensor) with torch.Tensor.scatter_reduce(..., "amax", include_self=False) standing in
for torch_scatter.scatter_max.  Both results are compared before anything is timed.

Also, per level, scatter_max alone (the three kernels of bsr_scatter_max with the level's index and row_map): the bytes
the call has to move, computed from the shapes, over its time, beside the box's copy rate measured here the way
tools/microbench/hbm_rates.py measures it.  And, unless --no-atomics, the rate of the 64-bit integer atomic maxima the
design rests on: scatter_max at 10^6 rows x 50 columns with one row, about ten rows and about a thousand rows a group.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
from functools import reduce

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.densify import grow_candidates, scatter_max  # noqa: E402

VOXEL_SIZE, SIZE_FACTORS = 0.001, (16, 4, 1)   # arguments.py:9-12 -> GM:826-827


def make_scene(N, K, F, seed):
    """Anchors on a noisy height field voxelised at VOXEL_SIZE (what create_from_pcd leaves), offsets a few voxels
    around them, a 5 % candidate mask."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xy = torch.rand(N, 2, device="cuda", generator=g) * 0.6
    z = 0.1 * torch.sin(9.0 * xy[:, :1]) * torch.cos(7.0 * xy[:, 1:]) + 0.002 * torch.randn(N, 1, device="cuda", generator=g)
    anchor = torch.round(torch.cat([xy, z], 1) / VOXEL_SIZE) * VOXEL_SIZE
    all_xyz = anchor.unsqueeze(1) + 0.005 * torch.randn(N, K, 3, device="cuda", generator=g)
    mask = torch.rand(N * K, device="cuda", generator=g) < 0.05
    feat = torch.randn(N, F, device="cuda", generator=g)
    return anchor, all_xyz, mask, feat


@torch.no_grad()
def eager_grow(anchor, all_xyz, candidate_mask, anchor_feat, cur_size, n_offsets):
    """GM:829-862, names as there."""
    feat_dim = anchor_feat.shape[1]
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


def time_alternating(fns, steps, warmup):
    """Median milliseconds of each callable, timed with events, one call of each in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms]


def copy_rate_tbps():
    """Read + write bytes per second of a 256 MB device copy (tools/microbench/hbm_rates.py: copy_read_plus_write)."""
    n = 256 * 1024 * 1024 // 4
    a, b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    (ms,) = time_alternating([lambda: b.copy_(a)], 30, 5)
    return 2 * n * 4 / (ms * 1e-3) / 1e12


def scatter_bytes(E, F, G, with_row_map):
    """What bsr_scatter_max has to move: the fill (8 G F), the pack pass (index and row_map once per row, the source
    value and one 8-byte atomic per element), the unpack pass (8 G F read, the winner's 4 bytes, 4 + 8 G F written)."""
    return 8 * G * F + E * (8 + (8 if with_row_map else 0)) + E * F * (4 + 8) + G * F * (8 + 4 + 4 + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--anchors", type=int, default=100_000)
    ap.add_argument("--no-atomics", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify needs the GPU: there is no CPU path and no timing without one")
    N, K, F = args.anchors, 10, 50
    anchor, all_xyz, mask, feat = make_scene(N, K, F, seed=0)
    copy_tbps = copy_rate_tbps()
    levels = []
    for factor in SIZE_FACTORS:
        cur_size = VOXEL_SIZE * factor
        want = eager_grow(anchor, all_xyz, mask, feat, cur_size, K)
        got = grow_candidates(anchor, all_xyz, mask, feat, cur_size)
        same = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
        native_ms, eager_ms = time_alternating([lambda: grow_candidates(anchor, all_xyz, mask, feat, cur_size),
                                                lambda: eager_grow(anchor, all_xyz, mask, feat, cur_size, K)],
                                               args.steps, args.warmup)
        # the scatter alone, on the level's index
        selected = mask.nonzero().squeeze(1)
        coords = torch.round(all_xyz.view(-1, 3)[selected] / cur_size).int()
        unique_coords, inverse = torch.unique(coords, return_inverse=True, dim=0)
        E, G = selected.shape[0], unique_coords.shape[0]
        row_map = selected // K
        (scatter_ms,) = time_alternating([lambda: scatter_max(feat, inverse, G, row_map=row_map)], args.steps, args.warmup)
        nbytes = scatter_bytes(E, F, G, True)
        levels.append({"cur_size": cur_size, "candidates": E, "unique_voxels": G, "new_anchors": int(got[0].shape[0]),
                       "same_result": same, "grow_candidates_ms": round(native_ms, 4), "eager_ms": round(eager_ms, 4),
                       "eager_over_native": round(eager_ms / native_ms, 2), "scatter_max_ms": round(scatter_ms, 4),
                       "scatter_bytes": nbytes, "scatter_TBps": round(nbytes / (scatter_ms * 1e-3) / 1e12, 4),
                       "scatter_share_of_copy_rate": round(nbytes / (scatter_ms * 1e-3) / 1e12 / copy_tbps, 4)})
    result = {"metric": "densify_grow_candidates_ms", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "anchors": N, "offsets": K, "features": F,
              "copy_read_plus_write_TBps": round(copy_tbps, 2), "levels": levels}
    if not args.no_atomics:
        E = 1_000_000
        g = torch.Generator(device="cuda").manual_seed(1)
        src = torch.randn(E, F, device="cuda", generator=g)
        atomics = []
        for G, name in ((E, "one_row_a_group"), (E // 10, "ten_rows_a_group"), (E // 1000, "thousand_rows_a_group")):
            index = torch.randperm(E, device="cuda", generator=g) % G
            (ms,) = time_alternating([lambda: scatter_max(src, index, G)], args.steps, args.warmup)
            atomics.append({"groups": G, "contention": name, "scatter_max_ms": round(ms, 4),
                            "atomic_max_u64_per_us": round(E * F / (ms * 1e3), 1),
                            "scatter_TBps": round(scatter_bytes(E, F, G, False) / (ms * 1e-3) / 1e12, 3)})
        result["atomic_max_u64"] = {"rows": E, "columns": F, "note": "whole call: fill + pack + unpack", "cases": atomics}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
