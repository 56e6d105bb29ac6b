"""Time the fused Adam step (include/bloomscene_adam.h, bloomscene_amd.optim.Adam) against the three forms of
torch.optim.Adam it can replace, at BloomScene's shape: the optimizer of scene/gaussian_model.py:531 over the seven per-anchor
tensors (F = 50, K = 10: 104 floats an anchor; opacity and rotation never receive a gradient), the four shipped hash tables
(12 3-D levels at 2^19, 3 x 4 2-D levels at 2^17, two features: about 10 M parameters) and the five MLP stacks.

    python tools/bench_adam.py [--anchors 100000 15000] [--iters 20] [--repeats 11] [--warmup 3] [--lib other_build.so]

Per anchor count, five sides alternate in this process, each on its own copy of the same parameters and gradients: this
optimizer, this optimizer in its capturable form replayed from a graph, torch.optim.Adam as the reference constructs it
(torch's default, the foreach path), foreach=False and fused=True.  A time is the GPU time between two events around `iters`
back-to-back steps divided by `iters`, taken `repeats` times: the median, the spread (max - min) and the spread of the
middle half are reported, and beside them the host's time in a call (the wall time of the same loop before the wait: where it
is as large as the GPU time, the side is bound by the host).  Before anything is timed, one step of every side is compared
with this optimizer's.  Also printed: the ideal traffic (28 B an element: p, g, m, v read, p, m, v written) and each side's share of the 6.29 TB/s the
MI355X streams in a float4 copy.  --lib times another build of the library (make variant ...).  Prints one JSON line.
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

RES_3D = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
RES_2D = (130, 258, 514, 1026)
F, K = 50, 10
STREAM_TBPS = 6.29      # the float4 copy rate of the MI355X


def model_shapes(n):
    """-> [(group name, [shapes], has a gradient)] in the reference's group order (gaussian_model.py:512-529)."""
    from bloomscene_amd.mix_encoding import MixEncoding
    enc = MixEncoding(2, RES_3D, 19, RES_2D, 17)
    tables = [tuple(p.shape) for p in enc.parameters()]
    c = enc.output_dim

    def mlp(i, h, o):
        return [(h, i), (h,), (o, h), (o,)]

    return [("anchor", [(n, 3)], True), ("offset", [(n, K, 3)], True), ("mask", [(n, K, 1)], True),
            ("anchor_feat", [(n, F)], True), ("opacity", [(n, 1)], False), ("scaling", [(n, 6)], True),
            ("rotation", [(n, 4)], False), ("mlp_opacity", mlp(F + 4, F, K), True), ("mlp_cov", mlp(F + 4, F, 7 * K), True),
            ("mlp_color", mlp(F + 4, F, 3 * K), True), ("encoding_xyz", tables, True),
            ("mlp_grid", mlp(c, 2 * F, (F + 6 + 3 * K) * 2 + 3), True), ("mlp_deform", mlp(c, 2 * F, 2 * K), True)]


def make_side(shapes, values, grads, cls, **kw):
    groups, params = [], []
    k = 0
    for gi, (name, shs, has_grad) in enumerate(shapes):
        ps = []
        for _ in shs:
            p = torch.nn.Parameter(values[k].clone())
            p.grad = grads[k].clone() if has_grad else None
            ps.append(p)
            k += 1
        groups.append({"params": ps, "lr": 2.0 ** -(7 + gi % 4), "name": name})     # fp32 values: both of our forms agree
        params += ps
    return params, cls(groups, lr=0.0, eps=1e-15, **kw)


def time_alternating(fns, iters, repeats, warmup):
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
            host[k].append((time.perf_counter() - t0) * 1e3 / iters)    # the host's share: the calls return before the GPU is done
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    return [(round(float(np.median(t)), 4), round(float(max(t) - min(t)), 4),
             round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4), round(float(np.median(h)), 4))
            for t, h in zip(times, host)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, nargs="+", default=[100_000, 15_000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam needs the GPU: there is no CPU path and no timing without one")
    if args.lib:
        from bloomscene_amd import _capi
        _capi.use_library(args.lib)
    from bloomscene_amd.optim import Adam
    gen = torch.Generator("cuda").manual_seed(0)
    result = {"metric": "adam_step_ms", "device": torch.cuda.get_device_name(0), "library": args.lib or "product",
              "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup, "stream_tbps": STREAM_TBPS, "sizes": {}}
    for n in args.anchors:
        shapes = model_shapes(n)
        flat = [s for _, shs, _ in shapes for s in shs]
        values = [torch.randn(s, device="cuda", generator=gen) for s in flat]
        grads = [torch.randn(s, device="cuda", generator=gen) * 1e-2 for s in flat]
        sides = {"fused_hip": make_side(shapes, values, grads, Adam),
                 "fused_hip_graph": make_side(shapes, values, grads, Adam, capturable=True),
                 "torch_default": make_side(shapes, values, grads, torch.optim.Adam),
                 "torch_foreach_false": make_side(shapes, values, grads, torch.optim.Adam, foreach=False),
                 "torch_fused": make_side(shapes, values, grads, torch.optim.Adam, fused=True)}
        # one step of every side against this optimizer's, before anything is timed
        for _, opt in sides.values():
            opt.step()
        torch.cuda.synchronize()
        ours = sides["fused_hip"][0]
        agree = {}
        for name, (params, _) in sides.items():
            if name == "fused_hip":
                continue
            agree[name] = {"bit_equal": all(bool(torch.equal(a, b)) for a, b in zip(params, ours)),
                           "max_diff": max(float((a - b).abs().max()) for a, b in zip(params, ours))}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sides["fused_hip_graph"][1].step()
        fns = [graph.replay if name == "fused_hip_graph" else opt.step for name, (_, opt) in sides.items()]
        timed = time_alternating(fns, args.iters, args.repeats, args.warmup)
        stepped = sum(int(np.prod(s)) for _, shs, has_grad in shapes if has_grad for s in shs)
        ideal_ms = 28 * stepped / (STREAM_TBPS * 1e12) * 1e3
        row = {"tensors_stepped": sum(len(shs) for _, shs, g in shapes if g), "elements_stepped": stepped,
               "ideal_bytes": 28 * stepped, "ideal_ms": round(ideal_ms, 4), "agreement_with_fused_hip_after_one_step": agree}
        for name, (ms, spread, iqr, host_ms) in zip(sides, timed):
            row[name] = {"ms": ms, "spread_ms": spread, "middle_half_spread_ms": iqr, "host_call_ms": host_ms,
                         "share_of_stream_rate": round(ideal_ms / ms, 3)}
        for name in ("torch_default", "torch_foreach_false", "torch_fused"):
            row[f"{name}_over_fused_hip"] = round(row[name]["ms"] / row["fused_hip"]["ms"], 2)
        result["sizes"][str(n)] = row
        del sides, graph, values, grads
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
