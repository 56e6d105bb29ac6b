"""Time the fused anchor heads (include/bloomscene_heads.h, bloomscene_amd.heads.anchor_heads_tensors) against the eager
lines they replace -- gaussian_renderer/__init__.py:151-154 and :168-185 over the three nn.Sequential heads of
scene/gaussian_model.py:234-252 -- at BloomScene's shape (feat_dim 50, 10 offsets) for 10 k and 100 k visible anchors.

    python tools/bench_heads.py [--anchors 10000 100000] [--iters 20] [--repeats 15] [--warmup 5]

Two sides, alternating in this process on the same tensors, each as forward alone (no_grad) and as forward + backward to
feat, anchor, the offset mask and the twelve weights:
  fused   one kernel forward; row pass + range sums + their addition backward
  eager   the lines as written (norm, division, cat, six Linear, ReLU / Tanh / Sigmoid, the mask product) and autograd
A time is the GPU time between two events around `iters` back-to-back iterations, divided by `iters`; it is taken
`repeats` times, the median is reported and beside it the spread (max - min over the repeats) and the spread of the
middle half of the repeats (75th - 25th percentile: what a shared box leaves of it).  The outputs and gradients
of the two sides are compared before anything is timed.  Also printed: the algorithmic FLOP and bytes of the shape and the
share of the fp32 vector peak (157.3 TFLOP/s) the fused times amount to.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.heads import anchor_heads_maps, anchor_heads_tensors  # noqa: E402

FP32_PEAK = 157.3e12


def eager_heads(feat, anchor, cam, weights, K, mask, gate=None):
    """The eager lines; ``gate [n, 3 F]`` (0 / 1) replaces relu(pre1) by pre1 * gate (for the agreement check only)."""
    n, F = feat.shape
    ob_view = anchor - cam
    ob_dist = ob_view.norm(dim=1, keepdim=True)
    ob_view = ob_view / ob_dist
    cat = torch.cat([feat, ob_view, ob_dist], dim=1)
    pre2 = []
    for h in range(3):
        W1, b1, W2, b2 = weights[4 * h:4 * h + 4]
        pre1 = torch.nn.functional.linear(cat, W1, b1)
        hid = torch.relu(pre1) if gate is None else pre1 * gate[:, h * F:(h + 1) * F]
        pre2.append(torch.nn.functional.linear(hid, W2, b2))
    neural_opacity = torch.tanh(pre2[0]).reshape(-1, 1) * mask.view(-1, 1)
    color = torch.sigmoid(pre2[2]).reshape(n * K, 3)
    scale_rot = pre2[1].reshape(n * K, 7)
    return neural_opacity, color, scale_rot


def make_inputs(n, F, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    weights = []
    for outputs in (1, 7, 3):
        for shape, fan in (((F, F + 4), F + 4), ((F,), F + 4), ((outputs * K, F), F), ((outputs * K,), F)):
            weights.append(((torch.rand(*shape, device="cuda", generator=g) * 2 - 1) / fan ** 0.5).requires_grad_(True))
    feat = torch.randn(n, F, device="cuda", generator=g).requires_grad_(True)
    anchor = (torch.randn(n, 3, device="cuda", generator=g) * 2).requires_grad_(True)
    cam = torch.tensor([0.3, -0.2, 4.0], device="cuda")
    mask = (torch.rand(n, K, 1, device="cuda", generator=g) < 0.7).float().requires_grad_(True)
    ups = [torch.randn(n * K, c, device="cuda", generator=g) for c in (1, 3, 7)]
    return feat, anchor, cam, weights, mask, ups


def time_alternating(fns, iters, repeats, warmup):
    """Per callable: (median ms per iteration, spread = max - min over the repeats, spread of the middle half)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    return [(round(float(np.median(t)), 4), round(float(max(t) - min(t)), 4),
             round(float(np.percentile(t, 75) - np.percentile(t, 25)), 4)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_heads needs the GPU: there is no CPU path and no timing without one")
    F, K = 50, 10
    result = {"metric": "anchor_heads_ms", "device": torch.cuda.get_device_name(0), "feat_dim": F, "offsets": K,
              "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup, "sizes": {}}
    for n in args.anchors:
        feat, anchor, cam, weights, mask, ups = make_inputs(n, F, K, seed=0)
        leaves = [feat, anchor, mask] + weights

        def fused():
            return anchor_heads_tensors(feat, anchor, cam, weights, K, offset_mask=mask)

        def eager():
            return eager_heads(feat, anchor, cam, weights, K, mask)

        def step(fn):
            def run():
                outs = fn()
                return outs, torch.autograd.grad(outs, leaves, ups)
            return run

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        # the eager side of the agreement check runs with the fused call's own ReLU gate (pre1 > 0): a hidden
        # pre-activation within rounding of 0 falls on the other side in a GEMM's order and moves a whole row's gradient
        with torch.no_grad():
            gate = (anchor_heads_maps(feat, anchor, cam, weights, K, offset_mask=mask)[3] > 0).float()

        def eager_gated():
            return eager_heads(feat, anchor, cam, weights, K, mask, gate)

        (fo, fg), (eo, eg), (_, ug) = step(fused)(), step(eager_gated)(), step(eager)()
        torch.cuda.synchronize()
        scale = lambda a, b: float((a - b).detach().abs().max()) / max(float(b.detach().abs().max()), 1e-30)
        agree = {"max_output_diff_over_scale": max(scale(a, b) for a, b in zip(fo, eo)),
                 "max_gradient_diff_over_scale": max(scale(a, b) for a, b in zip(fg, eg)),
                 "max_gradient_diff_over_scale_with_eager_own_gate": max(scale(a, b) for a, b in zip(fg, ug)),
                 "gates_that_differ": int(((torch.nn.functional.linear(
                     torch.cat([feat, (anchor - cam) / (anchor - cam).norm(dim=1, keepdim=True),
                                (anchor - cam).norm(dim=1, keepdim=True)], 1), torch.cat(weights[0::4]),
                     torch.cat(weights[1::4])) > 0).float() != gate).sum())}
        if not all(bool(torch.isfinite(t).all()) for t in fo + fg):
            raise SystemExit("bench_heads: the fused outputs or gradients are not finite")
        sides = {"fused_forward": forward_only(fused), "eager_forward": forward_only(eager),
                 "fused_forward_backward": step(fused), "eager_forward_backward": step(eager)}
        timed = time_alternating(list(sides.values()), args.iters, args.repeats, args.warmup)
        row = {name: {"ms": ms, "spread_ms": spread, "middle_half_spread_ms": iqr} for name, (ms, spread, iqr) in zip(sides, timed)}
        # algorithmic work: 2 FLOP per weight and row forward; the backward recomputes layer 1 and opacity's layer 2, and
        # forms dhid, dX and the two weight-gradient products
        w1, w2 = 3 * F * (F + 4), 11 * K * F
        flop_fwd = 2.0 * n * (w1 + w2)
        flop_bwd = 2.0 * n * (w1 + K * F) + 2.0 * n * (w2 + w1) + 2.0 * n * (w1 + w2)
        bytes_fwd = 4.0 * n * (F + 3 + K + 11 * K)
        bytes_bwd = 4.0 * n * (F + 3 + K + 3 * K + 11 * K + F + 3 + K)
        # what the fused backward moves on top of that: the per-row operands of the weight sums, written and read once
        scratch_rows = 2.0 * 4.0 * n * ((F + 4 + 3) // 4 * 4 + 4 + 2 * ((3 * F + 3) // 4 * 4 + 4) + (11 * K + 3) // 4 * 4 + 4)
        row["algorithmic"] = {
            "forward_gflop": round(flop_fwd / 1e9, 3), "forward_backward_gflop": round((flop_fwd + flop_bwd) / 1e9, 3),
            "forward_mbytes": round(bytes_fwd / 1e6, 2), "forward_backward_mbytes": round((bytes_fwd + bytes_bwd) / 1e6, 2),
            "fused_backward_scratch_round_trip_mbytes": round(scratch_rows / 1e6, 2),
            "fused_forward_share_of_fp32_peak": round(flop_fwd / (row["fused_forward"]["ms"] * 1e-3) / FP32_PEAK, 4),
            "fused_forward_backward_share_of_fp32_peak":
                round((flop_fwd + flop_bwd) / (row["fused_forward_backward"]["ms"] * 1e-3) / FP32_PEAK, 4)}
        row["agreement_with_eager"] = agree
        row["eager_over_fused_forward"] = round(row["eager_forward"]["ms"] / row["fused_forward"]["ms"], 2)
        row["eager_over_fused_forward_backward"] = round(row["eager_forward_backward"]["ms"] / row["fused_forward_backward"]["ms"], 2)
        result["sizes"][str(n)] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
