"""Time mean_dist3 (include/bloomscene_knn.h, BloomScene's distCUDA2) on three distributions at 10^5, 10^6 and 4 10^6
points: a uniform cube, a BloomScene-like cloud (noisy depth surfaces, planar pieces, ~5 % exact duplicates, voxelised
at 0.001) and tight clusters.

    python tools/bench_knn.py [--steps 10] [--warmup 3] [--sizes 100000,1000000,4000000] [--no-baselines]

Prints one JSON line: per (P, distribution) the median milliseconds of one call over `steps` calls timed with events
after `warmup` calls, and Mpoints/s.  Baselines, each timed once after a small warm-up: a chunked brute force in torch on
the GPU (|q|^2 + |p|^2 - 2 q.p by matmul, then topk; uniform cloud, P <= 10^6 only: its cost does not depend on the
distribution), and scipy's cKDTree(...).query(k=4, workers=16) on the CPU (build + query).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bloomscene_amd.knn import mean_dist3  # noqa: E402
import knn_reference as KR  # noqa: E402

KINDS = ("uniform", "surface", "clusters")


def time_gpu(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def brute_force(x, chunk=2048):
    """Baseline: squared distances by matmul, 4 smallest (self included), mean of the 3 others."""
    sq = (x * x).sum(1)
    out = torch.empty(x.shape[0], device=x.device)
    for a in range(0, x.shape[0], chunk):
        q = x[a:a + chunk]
        d = sq[a:a + chunk, None] + sq[None, :] - 2.0 * (q @ x.T)
        out[a:a + chunk] = torch.topk(d, 4, dim=1, largest=False).values[:, 1:].clamp_min(0).mean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    cases = []
    for P in sizes:
        for kind in KINDS:
            x_np = KR.make_cloud(kind, P, seed=0)
            x = torch.from_numpy(x_np).cuda()
            ms = time_gpu(lambda: mean_dist3(x), args.steps, args.warmup)
            case = {"P": P, "dist": kind, "ms": round(ms, 4), "mpoints_per_s": round(P / ms / 1e3, 1)}
            if not args.no_baselines:
                if kind == "uniform" and P <= 1_000_000:
                    brute_force(x[:4096])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    brute_force(x)
                    torch.cuda.synchronize()
                    case["torch_brute_force_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                try:
                    from scipy.spatial import cKDTree
                    t0 = time.perf_counter()
                    cKDTree(x_np).query(x_np, k=4, workers=16)
                    case["ckdtree_16cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                except ImportError:
                    case["ckdtree_16cpu_ms"] = None
            cases.append(case)
            del x
    print(json.dumps({"metric": "knn_mean_dist3_ms", "device": torch.cuda.get_device_name(0), "steps": args.steps,
                      "warmup": args.warmup, "cases": cases}))


if __name__ == "__main__":
    main()
