"""Time the fused depth-prior loss (include/bloomscene_depth_loss.h, bloomscene_amd.depth_loss.depth_prior_loss) against
the eager lines it replaces -- bloomscene.py:298-325 over utils/loss.py:26-80,170-202, restated -- forward + backward, at
BloomScene's [512, 512] and at [1080, 1920].

    python tools/bench_depth_prior.py [--steps 100] [--warmup 10]

One step is the three weighted terms and their gradient to the rendered depth.  Two sides, alternating in this process on
the same tensors after the warm-up of both:
  fused   depth_prior_loss: three kernels forward, two backward (plus the tickets' memsets)
  eager   the two min/max normalisations, HuberL1 with its boolean-mask assignment, CMD with its four .any() asserts
          and its moment loop, bilateral_filter through pad + unfold, and autograd
Per side: the GPU time between two events around the step, the host time until the step's calls have returned, and the
host time until the device has finished, each the median over `steps`; and the GPU time per step of `steps` steps
enqueued back to back between ONE pair of events.  The values of the two sides are compared before anything is timed.
Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.depth_loss import depth_prior_loss  # noqa: E402

WEIGHTS = (0.1, 0.1, 0.1)     # dep_value_lbd, dep_domin_lbd, dep_smooth_lbd
SHAPES = ((512, 512), (1080, 1920))


def eager_normalise(depth):
    hi, lo = depth.max(), depth.min()
    return (depth - lo) / (hi - lo + 1e-8)


def eager_huber(pred, gt, rgb, H, W, tresh=0.2):
    """utils/loss.py:181-200 with pred [1, H, W, 1], gt [1, H, W, 1], rgb [1, H, W, 3]; the reshape is to the call's H, W."""
    l1 = torch.abs(pred - gt)
    d = tresh * torch.max(l1)
    loss = ((pred - gt) ** 2 + d ** 2) / (2 * d)
    loss[l1 >= d] = l1[l1 >= d]
    gx = torch.mean(torch.abs(rgb[..., :, :-1, :] - rgb[..., :, 1:, :]), -1, keepdim=True)
    gy = torch.mean(torch.abs(rgb[..., :-1, :, :] - rgb[..., 1:, :, :]), -1, keepdim=True)
    loss = loss.reshape(H, W).unsqueeze(0).unsqueeze(-1)
    return (torch.exp(-gx) * loss[..., :, :-1, :]).mean() + (torch.exp(-gy) * loss[..., :-1, :, :]).mean()


def eager_matchnorm(a, b):
    power = torch.clamp(torch.pow(torch.abs(a - b) + 1e-6, 2), max=1e6)
    return torch.sqrt(torch.clamp(torch.sum(power), max=1e6) + 1e-6)


def eager_cmd(x1, x2, n_moments=5):
    """utils/loss.py:30-47, the four asserts (four host waits) included."""
    x1 = torch.clamp(x1, min=-1e6, max=1e6)
    x2 = torch.clamp(x2, min=-1e6, max=1e6)
    assert not torch.isnan(x1).any()
    assert not torch.isinf(x1).any()
    assert not torch.isnan(x2).any()
    assert not torch.isinf(x2).any()
    m1, m2 = torch.mean(x1, 0), torch.mean(x2, 0)
    s1, s2 = x1 - m1, x2 - m2
    total = eager_matchnorm(m1, m2)
    for k in range(2, n_moments + 1):
        total = total + eager_matchnorm(torch.mean(torch.pow(torch.abs(s1) + 1e-6, k), 0),
                                        torch.mean(torch.pow(torch.abs(s2) + 1e-6, k), 0))
    return total / x1.shape[0]


def eager_bilateral(depth, spatial_sigma=2.0, color_sigma=5.0, k=5):
    """utils/loss.py:63-80 with depth [1, H, W]."""
    B, H, W = depth.shape
    x = torch.arange(k, dtype=torch.float32).to(depth.device) - k // 2
    y = x.unsqueeze(0).expand(k, k)
    sk = torch.exp(-(y ** 2 + y.t() ** 2) / (2 * spatial_sigma ** 2))
    sk = sk / sk.sum()
    padded = F.pad(depth, (k // 2,) * 4, mode="replicate").unsqueeze(1)
    taps = F.unfold(padded, kernel_size=k).view(B, 1, k, k, H, W).permute(0, 4, 5, 1, 2, 3).squeeze(3)
    delta = depth.unsqueeze(3).unsqueeze(4) - taps
    colour = torch.exp(-delta.abs() / (2 * color_sigma ** 2))
    return torch.sum(sk * colour * delta ** 2, dim=(3, 4)).mean()


def eager_loss(render_depth, prior_depth, rgb, wv, wd, ws):
    """bloomscene.py:298-325: render_depth [1, H, W], prior_depth [H, W], rgb [H, W, 3] (the view the caller made)."""
    H, W = prior_depth.shape
    o = eager_normalise(prior_depth)
    r = eager_normalise(render_depth)
    loss = wv * eager_huber(r.unsqueeze(-1), o.unsqueeze(0).unsqueeze(-1), rgb.unsqueeze(0), H, W)
    loss = loss + wd * eager_cmd(r.unsqueeze(0), o.unsqueeze(0).unsqueeze(0))
    return loss + ws * eager_bilateral(r, spatial_sigma=2.0, color_sigma=5.0)


def time_alternating(fns, steps, warmup):
    """Per callable: median GPU ms between events, host ms until the calls returned, host ms until the device finished."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    gpu, host, done = ([[] for _ in fns] for _ in range(3))
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            t1 = time.perf_counter()
            b.synchronize()
            t2 = time.perf_counter()
            gpu[k].append(a.elapsed_time(b))
            host[k].append((t1 - t0) * 1e3)
            done[k].append((t2 - t0) * 1e3)
    return [tuple(round(float(np.median(v[k])), 4) for v in (gpu, host, done)) for k in range(len(fns))]


def time_back_to_back(fns, steps, rounds=3):
    """Per callable: GPU ms per step of `steps` steps between one pair of events; the median of `rounds`, alternating."""
    per = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            per[k].append(a.elapsed_time(b) / steps)
    return [round(float(np.median(v)), 4) for v in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_prior needs the GPU: there is no CPU path and no timing without one")
    wv, wd, ws = WEIGHTS
    result = {"metric": "depth_prior_loss_forward_backward_ms", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "weights": WEIGHTS, "shapes": {}}
    for H, W in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(0)
        prior = 1.0 + 4.0 * torch.rand((H, W), device="cuda", generator=gen)
        depth = (prior + 0.3 * torch.randn((H, W), device="cuda", generator=gen)).clamp(min=0.1)
        depth[: H // 4, : W // 4] = 0.0                       # pixels the rasterizer left empty: tied minima
        depth = depth.unsqueeze(0).requires_grad_(True)       # render_pkg["depth"]: [1, H, W]
        gt_image = torch.rand((3, H, W), device="cuda", generator=gen)
        rgb = gt_image.permute(1, 2, 0)                       # (upright; the reference's permute(2, 1, 0) needs H = W)

        def fused():
            loss = depth_prior_loss(depth, prior, rgb, value=wv, domin=wd, smooth=ws)
            grad, = torch.autograd.grad(loss, [depth])
            return loss, grad

        def eager():
            loss = eager_loss(depth, prior, rgb, wv, wd, ws)
            grad, = torch.autograd.grad(loss, [depth])
            return loss, grad

        sides = {"fused": fused, "eager": eager}
        print(f"bench_depth_prior: {(H, W)}: first calls", file=sys.stderr, flush=True)
        (loss_f, grad_f), (loss_e, grad_e) = fused(), eager()
        torch.cuda.synchronize()
        if not (math.isfinite(float(loss_f.detach())) and bool(torch.isfinite(grad_f).all())):
            raise SystemExit(f"bench_depth_prior: the fused result is not finite at {(H, W)}")
        entry = {"loss": {"fused": float(loss_f.detach()), "eager": float(loss_e.detach())},
                 "max_gradient_diff_over_scale": float((grad_f - grad_e).abs().max()) / float(grad_e.abs().max())}
        if abs(entry["loss"]["fused"] - entry["loss"]["eager"]) > 1e-4 * abs(entry["loss"]["eager"]):
            raise SystemExit(f"bench_depth_prior: the two sides disagree at {(H, W)}: {entry}")
        print(f"bench_depth_prior: {(H, W)}: timing", file=sys.stderr, flush=True)
        timed = time_alternating(list(sides.values()), args.steps, args.warmup)
        train = time_back_to_back(list(sides.values()), args.steps)
        for name, (gpu_ms, host_ms, done_ms), per_step in zip(sides, timed, train):
            entry[name] = {"gpu_ms": gpu_ms, "host_ms_until_calls_return": host_ms, "host_ms_until_device_done": done_ms,
                           "gpu_ms_per_step_back_to_back": per_step}
        entry["eager_over_fused_gpu"] = round(entry["eager"]["gpu_ms"] / entry["fused"]["gpu_ms"], 2)
        entry["eager_over_fused_back_to_back"] = round(entry["eager"]["gpu_ms_per_step_back_to_back"]
                                                       / entry["fused"]["gpu_ms_per_step_back_to_back"], 2)
        result["shapes"][f"{H}x{W}"] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
