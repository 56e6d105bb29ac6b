"""Time the fused photometric loss (include/bloomscene_loss.h, bloomscene_amd.loss.photometric_loss) against the eager
lines it replaces -- bloomscene.py:285-286 over utils/loss.py:83-134, restated -- forward + backward, at BloomScene's
[3, 512, 512] and at [3, 1080, 1920].

    python tools/bench_photometric.py [--steps 200] [--warmup 20]

One step is the loss and its gradient to the image.  Two sides, alternating in this process on the same tensors after the
warm-up of both (the eager side's first calls pick their convolution algorithms there):
  fused   photometric_loss: one forward and one backward kernel (plus the ticket's memset)
  eager   l1_loss and ssim as written: five depthwise 11 x 11 conv2d calls, the elementwise chain, three means, and autograd
Per side: the GPU time between two events around the step, the host time until the step's calls have returned, and the
host time until the device has finished, each the median over `steps`; and the GPU time per step of `steps` steps
enqueued back to back between ONE pair of events (a window of many steps instead of one).  The values of the two sides
are compared before anything is timed.  Prints one JSON line.
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

from bloomscene_amd.loss import photometric_loss  # noqa: E402

LAMBDA = 0.2                                       # arguments.py: lambda_dssim
SHAPES = ((3, 512, 512), (3, 1080, 1920))


def eager_window(channels, device):
    """utils/loss.py:91-99."""
    gauss = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w = (gauss / gauss.sum()).unsqueeze(1)
    return w.mm(w.t()).float().unsqueeze(0).unsqueeze(0).expand(channels, 1, 11, 11).contiguous().to(device)


def eager_loss(img, gt, lam):
    """bloomscene.py:285-286 over utils/loss.py:83-84, :103-132 (the window is rebuilt and uploaded per call, as there)."""
    ch = img.size(-3)
    win = eager_window(ch, img.device).type_as(img)
    mu1 = F.conv2d(img, win, padding=5, groups=ch)
    mu2 = F.conv2d(gt, win, padding=5, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img * img, win, padding=5, groups=ch) - mu1_sq
    sigma2_sq = F.conv2d(gt * gt, win, padding=5, groups=ch) - mu2_sq
    sigma12 = F.conv2d(img * gt, win, padding=5, groups=ch) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return (1.0 - lam) * torch.abs(img - gt).mean() + lam * (1.0 - ssim_map.mean())


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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric needs the GPU: there is no CPU path and no timing without one")
    result = {"metric": "photometric_loss_forward_backward_ms", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "lambda_dssim": LAMBDA, "shapes": {}}
    for shape in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(0)
        gt = torch.rand(shape, device="cuda", generator=gen)
        img = (gt + 0.05 * torch.randn(shape, device="cuda", generator=gen)).clamp(0, 1).requires_grad_(True)

        def step(fn):
            def run():
                loss = fn(img, gt, LAMBDA)
                grad, = torch.autograd.grad(loss, [img])
                return loss, grad
            return run

        sides = {"fused": step(photometric_loss), "eager": step(eager_loss)}
        print(f"bench_photometric: {shape}: first calls", file=sys.stderr, flush=True)
        (loss_f, grad_f), (loss_e, grad_e) = sides["fused"](), sides["eager"]()
        torch.cuda.synchronize()
        if not (math.isfinite(float(loss_f.detach())) and bool(torch.isfinite(grad_f).all())):
            raise SystemExit(f"bench_photometric: the fused result is not finite at {shape}")
        entry = {"loss": {"fused": float(loss_f.detach()), "eager": float(loss_e.detach())},
                 "max_gradient_diff_over_scale": float((grad_f - grad_e).abs().max()) / float(grad_e.abs().max())}
        print(f"bench_photometric: {shape}: timing", file=sys.stderr, flush=True)
        timed = time_alternating(list(sides.values()), args.steps, args.warmup)
        train = time_back_to_back(list(sides.values()), args.steps)
        for name, (gpu_ms, host_ms, done_ms), per_step in zip(sides, timed, train):
            entry[name] = {"gpu_ms": gpu_ms, "host_ms_until_calls_return": host_ms, "host_ms_until_device_done": done_ms,
                           "gpu_ms_per_step_back_to_back": per_step}
        entry["eager_over_fused_gpu"] = round(entry["eager"]["gpu_ms"] / entry["fused"]["gpu_ms"], 2)
        entry["eager_over_fused_back_to_back"] = round(entry["eager"]["gpu_ms_per_step_back_to_back"]
                                                       / entry["fused"]["gpu_ms_per_step_back_to_back"], 2)
        result["shapes"]["x".join(map(str, shape))] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
