"""Time the anchor position coder (include/bloomscene_anchor_codec.h, bloomscene_amd/anchor_codec.py) and the whole scene
file (bloomscene_amd/scene_file.py) on a ``synthetic.anchor_scene`` of 100 k anchors, ``F = 32``, ``K = 10``, 70 % of the
offsets kept and every twentieth anchor pruned, with the reference's default ``mix_3D2D_encoding`` tables.

    python tools/bench_scene_file.py [--steps 10] [--warmup 2] [--anchors 100000]

Printed: ``encode_anchors`` and ``decode_anchors`` (host clock around a call that ends in its host read; the median over
``steps`` after ``warmup`` calls), ``save_scene`` and ``load_scene`` (the same, file I/O to a temporary directory included),
the anchors' bits per anchor against the 48 the reference reports and the 96 it writes, and the file's bytes per section.
The synthetic anchors are uniform in a frustum, NOT voxelised surface points: their gaps are the widest a scene of this
size has; ``tests/test_anchor_codec_cpu.py`` holds the figure of a voxelised surface scene.  Nothing in the reference does
this work in one place, so there is no ratio: the times are written down in docs/EXPERIMENTS.md.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from collections import OrderedDict

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd import anchor_codec, context, scene_file, synthetic  # noqa: E402
from bloomscene_amd.mix_encoding import MixEncoding  # noqa: E402


def make_model(n, F, K, seed):
    dev = "cuda"
    s = synthetic.anchor_scene(n, K, 512, 512, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    mask = (torch.rand(n, K, 1, generator=g) < 0.7).float()
    mask[::20] = 0.0
    lo, hi = s.anchor.min(dim=0)[0], s.anchor.max(dim=0)[0]          # update_anchor_bound (scene/gaussian_model.py:402-410)
    lo = torch.where(lo < 0, lo * 1.2, lo * 0.8)
    hi = torch.where(hi > 0, hi * 1.2, hi * 0.8)
    enc = MixEncoding(4, (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514), 13, (130, 258, 514, 1026), 15)
    mlp_grid = nn.Sequential(nn.Linear(enc.output_dim, 2 * F), nn.ReLU(True), nn.Linear(2 * F, context.outputs(F, K)))
    mlps = OrderedDict([("mlp_opacity", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, K), nn.Tanh())),
                        ("mlp_cov", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, 7 * K))),
                        ("mlp_color", nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, 3 * K), nn.Sigmoid()))])
    t = lambda x: x.to(dev)
    return dict(anchor=t(s.anchor), bound_min=t(lo), bound_max=t(hi), anchor_feat=t(torch.randn(n, F, generator=g)),
                offset=t(s.grid_offsets), scaling=t(s.grid_scaling), mask=t(mask), encoding=enc.to(dev),
                mlp_grid=mlp_grid.to(dev), mlps=OrderedDict((k, m.to(dev)) for k, m in mlps.items()), F=F, K=K)


def timed(fn, steps, warmup):
    """Median milliseconds of ``fn()``, a call that ends in a host read, between two device synchronisations."""
    out = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--anchors", type=int, default=100000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--offsets", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_file.py needs the GPU: there is no CPU path")
    torch.manual_seed(0)
    m = make_model(args.anchors, args.features, args.offsets, seed=0)
    stream, perm = anchor_codec.encode_anchors(m["anchor"], m["bound_min"], m["bound_max"])
    n = perm.numel()
    back = anchor_codec.decode_anchors(stream, n=n, return_keys=True)
    keys = anchor_codec.lattice_keys(m["anchor"], m["bound_min"], m["bound_max"])
    assert torch.equal(back[3], keys[perm])
    res = {"anchors": n, "F": args.features, "K": args.offsets,
           "anchor_stream_bytes": stream.numel(), "anchor_bits_per_anchor": round(8 * stream.numel() / n, 3),
           "reference_reported_bits_per_anchor": 48, "reference_written_bits_per_anchor": 96,
           "encode_anchors_ms": round(timed(lambda: anchor_codec.encode_anchors(m["anchor"], m["bound_min"], m["bound_max"]),
                                            args.steps, args.warmup), 4),
           "decode_anchors_ms": round(timed(lambda: anchor_codec.decode_anchors(stream, n=n), args.steps, args.warmup), 4)}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.bsrs")
        info = scene_file.save_scene(path, **m)
        res["save_scene_ms"] = round(timed(lambda: scene_file.save_scene(path, **m), args.steps, args.warmup), 3)
        res["load_scene_ms"] = round(timed(lambda: scene_file.load_scene(path, "cuda"), args.steps, args.warmup), 3)
        res.update(kept_anchors=info.n, file_bytes=info.file_bytes, header_bytes=info.header_bytes,
                   section_bytes=dict(info.sections))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
