"""Time the fused rate term (include/bloomscene_entropy.h, bloomscene_amd.entropy.context_rates) against the eager lines it
replaces -- gaussian_renderer/__init__.py:77-84 and :100-127 ("GR") over utils/entropy_models.py:10-50 ("EM") -- at
BloomScene's shape: 100 k visible anchors, feat_dim 50, 10 offsets, 5 % of the anchors chosen.

    python tools/bench_entropy.py [--steps 20] [--warmup 3] [--anchors 100000]

One step is forward + backward of bit_per_param to the attributes and the context.  Three sides, alternating in this
process on the same tensors:
  fused        context_rates: three forward and three backward kernels, no gather, no host read
  eager_host   the lines as written: 13 boolean-index gathers, Normal.cdf twice per call, and the lower bound's backward
               through numpy on the host (EM:43-50)
  eager_device the same with the lower bound's mask taken on the device (what eager torch costs without that round trip)
Per side: the GPU time between two events around the step, the host time until the step's calls have returned, and
the host time until the device has finished, each the median over `steps`.  The values of the three sides are compared
before anything is timed.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.entropy import context_rates  # noqa: E402

Q_FEAT, Q_SCALING, Q_OFFSETS = 0.25, 2.5e-4, 5e-2   # GR:52-54


class LowBoundHost(torch.autograd.Function):
    """EM:35-50 as written: the backward builds its mask with numpy on the host."""

    @staticmethod
    def forward(ctx, l):
        ctx.save_for_backward(l)
        return torch.clamp(l, min=1e-6)

    @staticmethod
    def backward(ctx, g):
        l, = ctx.saved_tensors
        out = g.clone()
        out[l < 1e-6] = 0
        keep = np.logical_or(l.cpu().numpy() >= 1e-6, g.cpu().numpy() < 0.0)       # device -> host, twice
        return out * torch.from_numpy(keep.astype(np.float32)).to(g.device)         # host -> device


class LowBoundDevice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.clamp(x, min=1e-6)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g * (x >= 1e-6).to(g.dtype)


def eager_bits(x, mean, scale, Q, x_mean, low_bound):
    """EM:14-31."""
    half_span = 15_000 * Q
    lo, hi = (x_mean - half_span).detach(), (x_mean + half_span).detach()
    xc = torch.clamp(x, min=lo, max=hi)
    normal = torch.distributions.normal.Normal(mean, torch.clamp(scale, min=1e-9), validate_args=False)
    lower, upper = normal.cdf(xc - 0.5 * Q), normal.cdf(xc + 0.5 * Q)
    return -torch.log2(low_bound.apply(torch.abs(upper - lower)))


def eager_rates(feat, grid_scaling, grid_offsets, context, choose, grid_masks, rate, feat_mean, scaling_mean, offsets_mean,
                feat_dim, K, low_bound):
    """GR:77-84, GR:100-127."""
    mean, scale, mean_s, scale_s, mean_o, scale_o, adj_f, adj_s, adj_o = torch.split(
        context, [feat_dim, feat_dim, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)
    Qf = Q_FEAT * (1 + torch.tanh(adj_f))
    Qs = Q_SCALING * (1 + torch.tanh(adj_s))
    Qo = Q_OFFSETS * (1 + torch.tanh(adj_o))
    feat_c, scaling_c, offsets_c = feat[choose], grid_scaling[choose], grid_offsets[choose].view(-1, 3 * K)
    mean, scale, mean_s, scale_s, mean_o, scale_o = (t[choose] for t in (mean, scale, mean_s, scale_s, mean_o, scale_o))
    Qf, Qs, Qo = Qf[choose], Qs[choose], Qo[choose]
    masks = grid_masks[choose].repeat(1, 1, 3).view(-1, 3 * K)
    bit_feat = eager_bits(feat_c, mean, scale, Qf, feat_mean, low_bound)
    bit_scaling = eager_bits(scaling_c, mean_s, scale_s, Qs, scaling_mean, low_bound)
    bit_offsets = eager_bits(offsets_c, mean_o, scale_o, Qo, offsets_mean, low_bound) * masks
    per_feat = torch.sum(bit_feat) / bit_feat.numel() * rate
    per_scaling = torch.sum(bit_scaling) / bit_scaling.numel() * rate
    per_offsets = torch.sum(bit_offsets) / bit_offsets.numel() * rate
    per_param = (torch.sum(bit_feat) + torch.sum(bit_scaling) + torch.sum(bit_offsets)) / \
        (bit_feat.numel() + bit_scaling.numel() + bit_offsets.numel()) * rate
    return per_param, per_feat, per_scaling, per_offsets


def make_inputs(n, feat_dim, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def randn(*s):
        return torch.randn(s, device="cuda", generator=g)

    widths = [feat_dim, feat_dim, 6, 6, 3 * K, 3 * K, 1, 1, 1]
    at = np.cumsum([0] + widths)
    context = randn(n, sum(widths))
    for i in (1, 3, 5):
        context[:, at[i]:at[i + 1]] = 0.3 * torch.exp(context[:, at[i]:at[i + 1]])
    context[:, at[2]:at[4]] *= 1e-3
    context[:, at[4]:at[6]] *= 0.2
    feat = (context[:, :feat_dim] + randn(n, feat_dim) * context[:, at[1]:at[2]]).contiguous()
    grid_scaling = (context[:, at[2]:at[3]] + randn(n, 6) * context[:, at[3]:at[4]]).contiguous()
    grid_offsets = (context[:, at[4]:at[5]] + randn(n, 3 * K) * context[:, at[5]:at[6]]).reshape(n, K, 3).contiguous()
    choose = torch.rand(n, device="cuda", generator=g) <= 0.05
    grid_masks = (torch.rand(n, K, 1, device="cuda", generator=g) < 0.6).float()
    rate = torch.tensor(0.9, device="cuda")
    return feat, grid_scaling, grid_offsets, context, choose, grid_masks, rate, feat.mean(), grid_scaling.mean(), grid_offsets.mean()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--anchors", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_entropy needs the GPU: there is no CPU path and no timing without one")
    n, feat_dim, K = args.anchors, 50, 10
    inputs = make_inputs(n, feat_dim, K, seed=0)
    leaves = [inputs[i].requires_grad_(True) for i in range(4)]   # feat, grid_scaling, grid_offsets, context

    def step(fn):
        def run():
            out = fn()
            grads = torch.autograd.grad(out[0], leaves)
            return out, grads
        return run

    sides = {
        "fused": step(lambda: context_rates(*inputs, feat_dim, K, Q_FEAT, Q_SCALING, Q_OFFSETS)),
        "eager_host": step(lambda: eager_rates(*inputs, feat_dim, K, LowBoundHost)),
        "eager_device": step(lambda: eager_rates(*inputs, feat_dim, K, LowBoundDevice)),
    }
    results = {name: fn() for name, fn in sides.items()}
    torch.cuda.synchronize()
    values = {name: [float(v.detach()) for v in out] for name, (out, _) in results.items()}
    ref_out, ref_grads = results["eager_device"]
    agree = {}
    for name in ("fused", "eager_host"):
        out, grads = results[name]
        agree[name] = {
            "max_rel_diff_of_the_four_rates": max(abs(float(a) - float(b)) / max(abs(float(b)), 1e-30) for a, b in zip(out, ref_out)),
            "max_gradient_diff_over_scale": max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
                                                for a, b in zip(grads, ref_grads)),
        }
    if not all(math.isfinite(v) for v in values["fused"]):
        raise SystemExit(f"bench_entropy: the fused rates are not finite: {values['fused']}")
    timed = time_alternating(list(sides.values()), args.steps, args.warmup)
    result = {"metric": "rate_term_forward_backward_ms", "device": torch.cuda.get_device_name(0), "steps": args.steps,
              "warmup": args.warmup, "anchors": n, "feat_dim": feat_dim, "offsets": K, "chosen": int(inputs[4].sum()),
              "bit_per_param": values, "agreement_with_eager_device": agree}
    for name, (gpu_ms, host_ms, done_ms) in zip(sides, timed):
        result[name] = {"gpu_ms": gpu_ms, "host_ms_until_calls_return": host_ms, "host_ms_until_device_done": done_ms}
    result["eager_host_over_fused_gpu"] = round(result["eager_host"]["gpu_ms"] / result["fused"]["gpu_ms"], 2)
    result["eager_host_over_fused_wall"] = round(result["eager_host"]["host_ms_until_device_done"]
                                                 / result["fused"]["host_ms_until_device_done"], 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
