"""Time the anchor adjustment (include/bloomscene_adjust.h) against what it replaces, at BloomScene's shapes.

    python tools/bench_adjust.py [--repeats 9] [--warmup 2] [--anchors 100000 15000] [--features 32 50]
                                 [--grow 0.01 0.05] [--prune 0.05] [--resize-iters 20]

Per shape (anchors x F, K = 10) and growth fraction, two sides alternate in this process:
    fused   bloomscene_amd.adjust.adjust_anchor
    eager   GM:898-952 in eager torch on the same device (tests/adjust_reference.eager_adjust)
on a model whose statistics prune about `prune` of the anchors and make about `grow` of the offsets candidates, with
bloomscene_amd.optim.Adam holding moments for five of the seven per-anchor groups.  The model is rebuilt from a saved copy
before every repetition, outside the timed region; both sides get the same random numbers and their results are compared
before anything is timed.  A figure is the wall time of the whole call with its host reads, start to the device being
idle again: the median of `repeats`, the spread (max - min), and beside them the host's time in the call (until it
returns).  resize_rows alone, on the tensors of the same adjustment, is timed as `resize-iters` back-to-back calls and set
against its ideal: the bytes it reads and writes at the 6.29 TB/s a float4 copy reaches on this box.
Prints one JSON line.
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

import adjust_reference as AR  # noqa: E402
from bloomscene_amd import adjust  # noqa: E402
from bloomscene_amd.optim import Adam  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s, float4 copy (read + write counted)
STATEFUL = ("anchor", "offset", "mask", "anchor_feat", "scaling")


def build(state, moments):
    """A fresh model on the device from the saved host state, the optimizer holding the saved moments at step 2."""
    model = AR.Model(state, "cuda", lambda groups: Adam(groups, lr=0.0, eps=1e-15))
    for g in model.optimizer.param_groups:
        if g["name"] in STATEFUL:
            m, v = moments[g["name"]]
            model.optimizer.state[g["params"][0]] = {"step": torch.tensor(2.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return model


def same(a, b):
    sa, sb = a.state(), b.state()
    ok = all(np.array_equal(sa["params"][n].view(np.uint32), sb["params"][n].view(np.uint32)) for n in AR.PARAMS)
    ok = ok and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for n in sa["moments"]
                    for x, y in zip(sa["moments"][n], sb["moments"][n]))
    return bool(ok and all(np.array_equal(sa[n], sb[n]) for n in ("opacity_accum", "anchor_demon", "offset_gradient_accum",
                                                                    "offset_denom")))


def summary(wall, host):
    return {"wall_ms": round(float(np.median(wall)), 3), "spread_ms": round(float(max(wall) - min(wall)), 3),
            "host_ms": round(float(np.median(host)), 3)}


def time_resize(model, rand, iters, repeats):
    """resize_rows alone on the adjustment's own tensors -> (median ms of one call, bytes moved)."""
    K, N = model.n_offsets, model._anchor.shape[0]
    thresholds = [0.0002 * ((model.update_hierachy_factor // 2) ** i) for i in range(model.update_depth)]
    offset_flags, anchor_flags, src_of, status = adjust.decide(model.opacity_accum, model.anchor_demon,
                                                               model.offset_gradient_accum, model.offset_denom, K, thresholds)
    n_keep = int(status[0])
    blocks = adjust.grow(model, offset_flags, rand)
    A = blocks["anchor"].shape[0]
    tensors, appends = [], []
    for g in model.optimizer.param_groups:
        if g["name"] not in AR.PARAMS:
            continue
        p = g["params"][0]
        tensors.append(p)
        appends.append(blocks.get(g["name"]))
        st = model.optimizer.state.get(p)
        if st:
            tensors += [st["exp_avg"], st["exp_avg_sq"]]
            appends += [None, None]
    tensors += [model.opacity_accum, model.anchor_demon, model.offset_gradient_accum.view(N, K), model.offset_denom.view(N, K)]
    appends += [None] * 4
    outs = [torch.empty((n_keep + A) * (t.numel() // N), dtype=torch.float32, device="cuda") for t in tensors]
    call = lambda: adjust.resize_rows(tensors, src_of, n_keep, appends, n_append=A, out=outs)
    moved = sum(4 * (t.numel() // N) * (n_keep + (A if a is not None else 0) + n_keep + A) for t, a in zip(tensors, appends))
    moved += 4 * n_keep * len(tensors)
    for _ in range(3):
        call()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return float(np.median(times)), moved, len(tensors), n_keep, A, int((offset_flags & 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--anchors", type=int, nargs="+", default=[100_000, 15_000])
    ap.add_argument("--features", type=int, nargs="+", default=[32, 50])
    ap.add_argument("--grow", type=float, nargs="+", default=[0.01, 0.05])
    ap.add_argument("--prune", type=float, default=0.05)
    ap.add_argument("--resize-iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adjust needs the GPU: there is no CPU path and no timing without one")
    K = 10
    result = {"metric": "adjust_anchor_ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "warmup": args.warmup, "offsets": K, "prune": args.prune, "cases": []}
    sides = {"fused": adjust.adjust_anchor, "eager": AR.eager_adjust}
    for N in args.anchors:
        for F in args.features:
            for grow in args.grow:
                # (make_state looks at 3 of 7 offset counts and 4 of 8 anchor counts: the fractions are of those)
                state = AR.make_state(N, F, K, seed=1, grow=grow * 7 / 3, prune=args.prune * 2, box=4.0 * (N / 2000) ** (1 / 3))
                gen = torch.Generator(device="cuda").manual_seed(2)
                moments = {n: tuple(torch.randn(state["params"][n].shape, device="cuda", generator=gen) * s for s in (0.01, 1e-4))
                           for n in STATEFUL}
                moments = {n: (m, v.abs()) for n, (m, v) in moments.items()}
                rand = [torch.rand(N * K, device="cuda", generator=gen) for _ in range(3)]
                models = {k: build(state, moments) for k in sides}
                for k, fn in sides.items():
                    fn(models[k], rand=rand)
                n_new = models["fused"]._anchor.shape[0]
                case = {"anchors": N, "features": F, "grow": grow, "anchors_after": n_new,
                        "same_as_eager": same(models["fused"], models["eager"])}
                wall, host = {k: [] for k in sides}, {k: [] for k in sides}
                for rep in range(args.warmup + args.repeats):
                    for k, fn in sides.items():
                        model = build(state, moments)                 # restored, outside the timed region
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(model, rand=rand)
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        if rep >= args.warmup:
                            wall[k].append((t2 - t0) * 1e3)
                            host[k].append((t1 - t0) * 1e3)
                for k in sides:
                    case[k] = summary(wall[k], host[k])
                case["eager_over_fused"] = round(case["eager"]["wall_ms"] / case["fused"]["wall_ms"], 2)
                ms, moved, n_tensors, n_keep, A, cand = time_resize(build(state, moments), rand, args.resize_iters, args.repeats)
                case["pruned"], case["level0_candidates_before_rand"] = N - n_keep, cand
                case["resize_rows"] = {"gpu_ms": round(ms, 4), "tensors": n_tensors, "n_keep": n_keep, "appended": A,
                                       "bytes": moved, "ideal_ms": round(moved / COPY_RATE * 1e3, 4),
                                       "over_ideal": round(ms / (moved / COPY_RATE * 1e3), 2)}
                result["cases"].append(case)
                print(f"anchors {N} F {F} grow {grow}: done", file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
