"""Time the fused context head (include/bloomscene_context.h, bloomscene_amd.context) against the eager lines it replaces
at BloomScene's shape (encoding width 48, hidden 100, feat_dim 50, 10 offsets) for 100 k visible anchors:

  training    gaussian_renderer/__init__.py:76-97: the grid MLP, the split, the three step sizes, the noise injection
  rendering   gaussian_renderer/__init__.py:133-142 without the two synchronize() calls: the grid MLP (all 175 outputs),
              the step sizes, STE_multistep on feat, grid_scaling, grid_offsets

    python tools/bench_context.py [--anchors 100000] [--iters 20] [--repeats 15] [--warmup 5]

Both sides run alternating in this process on the same tensors; the noise is drawn once and given to both (the caller keeps
the three randn_like lines either way), and so are the three means.  The training form is timed as forward alone (no_grad)
and as forward + backward to enc, the three attributes and the four weights; the rendering form has no gradient.  A time is
the GPU time between two events around `iters` back-to-back iterations, divided by `iters`; it is taken `repeats` times,
the median is reported and beside it the spread (max - min over the repeats) and the spread of the middle half of the
repeats.  The outputs and gradients of the two sides are compared before anything is timed.  Also printed: the algorithmic
FLOP of the shape and the share of the fp32 vector peak (157.3 TFLOP/s) the fused times amount to.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.context import (Q_DEFAULT, context_head_maps, context_head_tensors, context_quantise_tensors,  # noqa: E402
                                    outputs)

FP32_PEAK = 157.3e12


def eager_steps(enc, weights, F, K, gate=None):
    W1, b1, W2, b2 = weights
    pre1 = torch.nn.functional.linear(enc, W1, b1)
    hid = torch.relu(pre1) if gate is None else pre1 * gate
    feat_context = torch.nn.functional.linear(hid, W2, b2)
    adj = torch.split(feat_context, [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1], dim=-1)[-3:]
    return feat_context, [q * (1 + torch.tanh(a)) for q, a in zip(Q_DEFAULT, adj)]


def eager_training(enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, gate=None):
    """GR:76-97; ``gate [n, H]`` (0 / 1) replaces relu(pre1) by pre1 * gate (for the agreement check only)."""
    feat_context, (Q_feat, Q_scaling, Q_offsets) = eager_steps(enc, weights, F, K, gate)
    feat = feat + noise[0] * (Q_feat + 1e-6)
    grid_scaling = grid_scaling + noise[1] * (Q_scaling + 1e-6)
    grid_offsets = grid_offsets + noise[2] * (Q_offsets + 1e-6).unsqueeze(1)
    return feat_context, torch.cat([Q_feat, Q_scaling, Q_offsets], dim=1), feat, grid_scaling, grid_offsets


def ste_multistep(x, Q, x_mean):
    x = torch.clamp(x, min=(x_mean - 15_000 * Q).detach(), max=(x_mean + 15_000 * Q).detach())
    Q_q = torch.round(x / Q) * Q
    return Q_q + torch.tanh(x - Q_q) * Q


def eager_rendering(enc, weights, F, K, feat, grid_scaling, grid_offsets, means):
    """GR:133-142 (without the synchronize() calls)."""
    _, (Q_feat, Q_scaling, Q_offsets) = eager_steps(enc, weights, F, K)
    return (ste_multistep(feat, Q_feat, means[0]).detach(), ste_multistep(grid_scaling, Q_scaling, means[1]).detach(),
            ste_multistep(grid_offsets, Q_offsets.unsqueeze(1), means[2]).detach())


def make_inputs(n, D, H, F, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    O = outputs(F, K)
    weights = [((torch.rand(*shape, device="cuda", generator=g) * 2 - 1) / fan ** 0.5).requires_grad_(True)
               for shape, fan in (((H, D), D), ((H,), D), ((O, H), H), ((O,), H))]
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    enc = (rn(n, D) * 0.5).requires_grad_(True)
    feat = rn(n, F).requires_grad_(True)
    grid_scaling = torch.exp(rn(n, 6) * 0.8 - 1.0).requires_grad_(True)
    grid_offsets = (rn(n, K, 3) * 0.3).requires_grad_(True)
    noise = (rn(n, F), rn(n, 6), rn(n, K, 3))
    means = [t.detach().mean() for t in (feat, grid_scaling, grid_offsets)]
    ups = [rn(n, O), rn(n, 3), rn(n, F), rn(n, 6), rn(n, K, 3)]
    return enc, weights, feat, grid_scaling, grid_offsets, noise, means, ups


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
    ap.add_argument("--anchors", type=int, nargs="+", default=[100_000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_context needs the GPU: there is no CPU path and no timing without one")
    D, H, F, K = 48, 100, 50, 10
    O = outputs(F, K)
    result = {"metric": "context_head_ms", "device": torch.cuda.get_device_name(0), "encoding": D, "hidden": H, "feat_dim": F,
              "offsets": K, "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup, "sizes": {}}
    for n in args.anchors:
        enc, weights, feat, grid_scaling, grid_offsets, noise, means, ups = make_inputs(n, D, H, F, K, seed=0)
        leaves = [enc, feat, grid_scaling, grid_offsets] + weights
        frozen = [t.detach() for t in leaves]

        def fused():
            return context_head_tensors(enc, weights, F, K, feat, grid_scaling, grid_offsets, noise)

        def eager():
            return eager_training(enc, weights, F, K, feat, grid_scaling, grid_offsets, noise)

        def fused_rendering():
            return context_quantise_tensors(frozen[0], frozen[4:], F, K, *frozen[1:4], *means)

        def eager_render():
            with torch.no_grad():
                return eager_rendering(frozen[0], frozen[4:], F, K, *frozen[1:4], means)

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
            gate = (context_head_maps(*frozen[:1], frozen[4:], F, K)[5] > 0).float()

        def eager_gated():
            return eager_training(enc, weights, F, K, feat, grid_scaling, grid_offsets, noise, gate)

        (fo, fg), (eo, eg) = step(fused)(), step(eager_gated)()
        fq, eq = fused_rendering(), eager_render()
        torch.cuda.synchronize()
        scale = lambda a, b: float((a - b).detach().abs().max()) / max(float(b.detach().abs().max()), 1e-30)
        # the quantised values sit on a grid of Q: two sides whose Q differ in the last bits land on neighbouring steps in
        # a few elements, so the rendering form is compared in steps of Q
        Qcols = fo[1].detach()
        steps_off = max(float(((a - b).reshape(n, -1).abs() / Qcols[:, c:c + 1]).max()) for c, (a, b) in enumerate(zip(fq, eq)))
        agree = {"max_output_diff_over_scale": max(scale(a, b) for a, b in zip(fo, eo)),
                 "max_gradient_diff_over_scale": max(scale(a, b) for a, b in zip(fg, eg)),
                 "rendering_max_diff_in_steps_of_Q": steps_off}
        if not all(bool(torch.isfinite(t).all()) for t in list(fo) + list(fg) + list(fq)):
            raise SystemExit("bench_context: the fused outputs or gradients are not finite")
        sides = {"fused_forward": forward_only(fused), "eager_forward": forward_only(eager),
                 "fused_forward_backward": step(fused), "eager_forward_backward": step(eager),
                 "fused_rendering": fused_rendering, "eager_rendering": eager_render}
        timed = time_alternating(list(sides.values()), args.iters, args.repeats, args.warmup)
        row = {name: {"ms": ms, "spread_ms": spread, "middle_half_spread_ms": iqr} for name, (ms, spread, iqr) in zip(sides, timed)}
        # algorithmic work: 2 FLOP per weight and row forward; the backward recomputes layer 1 and three rows of layer 2 and
        # forms dhid, d enc and the two weight-gradient products; the rendering form is layer 1 and three rows of layer 2
        w1, w2 = H * D, O * H
        flop_fwd = 2.0 * n * (w1 + w2)
        flop_bwd = 2.0 * n * (w1 + 3 * H) + 2.0 * n * (w2 + w1) + 2.0 * n * (w1 + w2)
        flop_render = 2.0 * n * (w1 + 3 * H)
        row["algorithmic"] = {
            "forward_gflop": round(flop_fwd / 1e9, 3), "forward_backward_gflop": round((flop_fwd + flop_bwd) / 1e9, 3),
            "rendering_gflop": round(flop_render / 1e9, 3),
            "fused_forward_share_of_fp32_peak": round(flop_fwd / (row["fused_forward"]["ms"] * 1e-3) / FP32_PEAK, 4),
            "fused_forward_backward_share_of_fp32_peak":
                round((flop_fwd + flop_bwd) / (row["fused_forward_backward"]["ms"] * 1e-3) / FP32_PEAK, 4),
            "fused_rendering_share_of_fp32_peak": round(flop_render / (row["fused_rendering"]["ms"] * 1e-3) / FP32_PEAK, 4)}
        row["agreement_with_eager"] = agree
        for name in ("forward", "forward_backward", "rendering"):
            row[f"eager_over_fused_{name}"] = round(row[f"eager_{name}"]["ms"] / row[f"fused_{name}"]["ms"], 2)
        result["sizes"][str(n)] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
