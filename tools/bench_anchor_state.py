"""Time the fused anchor state (include/bloomscene_anchor_state.h, bloomscene_amd.anchor_state.visible / accumulate) against
the eager lines it replaces -- gaussian_renderer/__init__.py:34-46 over the model properties of
scene/gaussian_model.py:342-364 / :394-399, and GaussianModel.training_statis, scene/gaussian_model.py:742-759 -- at
100 k anchors, feat_dim 32, 10 offsets, with 15 % and with 100 % of the anchors visible.

    python tools/bench_anchor_state.py [--anchors 100000] [--visible 0.15 1.0] [--iters 20] [--repeats 15] [--warmup 5]

Sides, alternating in this process on the same tensors:
  A  fused / eager forward alone (no_grad), and forward + backward to the five [N, ...] inputs (dense gradients)
  B  fused / eager update of the four accumulators
A time is the GPU time between two events around `iters` back-to-back iterations, divided by `iters`; it is taken
`repeats` times, the median is reported and beside it the spread (max - min over the repeats) and the spread of the middle
half.  The outputs, gradients and accumulators of the two sides are compared before anything is timed.  Also printed: the
algorithmic bytes of each side (for the eager side: the operands of its elementwise passes and gathers, each read or
written once) and the share of the box's copy rate the fused times amount to -- the copy rate is measured here the way
tools/microbench/hbm_rates.py measures it (256 MB, read + write).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd.anchor_state import accumulate, visible  # noqa: E402

Q_ANCHOR = 1 / (2 ** 16 - 1)


class QuantizeAnchor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchors, min_v, max_v):
        interval = (max_v - min_v) * Q_ANCHOR + 1e-6
        q = torch.clamp(torch.div(anchors - min_v, interval, rounding_mode="floor"), 0, 2 ** 16 - 1)
        return q * interval + min_v

    @staticmethod
    def backward(ctx, g):
        return g, None, None


def eager_visible(visible_mask, anchor, bmin, bmax, feat, offset, scaling, mask):
    """The eager lines: every property over all N rows, then the boolean-mask gathers."""
    get_anchor = QuantizeAnchor.apply(anchor, bmin, bmax)
    a = get_anchor[visible_mask]
    f = feat[visible_mask]
    o = offset[visible_mask]
    s = (1.0 * torch.exp(scaling))[visible_mask]
    sig = torch.sigmoid(mask)
    m = (((sig > 0.01).float() - sig).detach() + sig)[visible_mask]
    with torch.no_grad():
        sig2 = torch.sigmoid(mask)
        full = ((sig2 > 0.01).float() - sig2).detach() + sig2
        mask_anchor = (torch.sum(full, dim=1)[:, 0] > 0)[visible_mask]
    rate = (mask_anchor.sum() / mask_anchor.numel()).detach()
    return a, f, o, s, m, mask_anchor.to(torch.bool), rate


def eager_accumulate(acc, anchor_visible_mask, opacity, selection, update_filter, grad, K):
    opacity_accum, anchor_demon, offset_gradient_accum, offset_denom = acc
    temp_opacity = opacity.clone().view(-1).detach()
    temp_opacity[temp_opacity < 0] = 0
    temp_opacity = temp_opacity.view([-1, K])
    opacity_accum[anchor_visible_mask] += temp_opacity.sum(dim=1, keepdim=True)
    anchor_demon[anchor_visible_mask] += 1
    anchor_visible_mask = anchor_visible_mask.unsqueeze(dim=1).repeat([1, K]).view(-1)
    combined_mask = torch.zeros_like(offset_gradient_accum, dtype=torch.bool).squeeze(dim=1)
    combined_mask[anchor_visible_mask] = selection
    temp_mask = combined_mask.clone()
    combined_mask[temp_mask] = update_filter
    grad_norm = torch.norm(grad[update_filter, :2], dim=-1, keepdim=True)
    offset_gradient_accum[combined_mask] += grad_norm
    offset_denom[combined_mask] += 1


def copy_rate():
    """bytes / s of a 256 MB device copy (read + write), as tools/microbench/hbm_rates.py takes it."""
    n = 256 * 1024 * 1024 // 4
    a, b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    for _ in range(5):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(30):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2 * n * 4 / (e0.elapsed_time(e1) / 30 * 1e-3)


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
    ap.add_argument("--anchors", type=int, default=100_000)
    ap.add_argument("--visible", type=float, nargs="+", default=[0.15, 1.0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_anchor_state needs the GPU: there is no CPU path and no timing without one")
    N, F, K = args.anchors, 32, 10
    rate = copy_rate()
    result = {"metric": "anchor_state_ms", "device": torch.cuda.get_device_name(0), "anchors": N, "feat_dim": F, "offsets": K,
              "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "copy_read_plus_write_TBps": round(rate / 1e12, 2), "visible": {}}
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    bmin, bmax = torch.tensor([[-3.0, -2.0, -1.0]], device="cuda"), torch.tensor([[3.0, 2.5, 4.0]], device="cuda")
    anchor = (bmin + (bmax - bmin) * torch.rand(N, 3, device="cuda", generator=g)).requires_grad_(True)
    feat, offset = rnd(N, F).requires_grad_(True), rnd(N, K, 3).requires_grad_(True)
    scaling = (rnd(N, 6) - 3).requires_grad_(True)
    mask = (rnd(N, K, 1) * 2 - 4.6)
    mask = torch.where((mask + 4.59512).abs() < 1e-3, mask + 2e-3, mask).requires_grad_(True)
    leaves = [anchor, feat, offset, scaling, mask]
    for share in args.visible:
        n = max(1, int(round(N * share)))
        idx = torch.sort(torch.randperm(N, device="cuda", generator=g)[:n]).values
        visible_mask = torch.zeros(N, dtype=torch.bool, device="cuda")
        visible_mask[idx] = True
        ups = [rnd(n, 3), rnd(n, F), rnd(n, K, 3), rnd(n, 6), rnd(n, K, 1)]

        def fused():
            return visible(idx, anchor, bmin, bmax, feat, offset, scaling, mask)

        def eager():
            return eager_visible(visible_mask, anchor, bmin, bmax, feat, offset, scaling, mask)

        def step(fn):
            def run():
                outs = fn()
                return outs, torch.autograd.grad(outs[:5], leaves, ups)
            return run

        def forward_only(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        (fo, fg), (eo, eg) = step(fused)(), step(eager)()
        torch.cuda.synchronize()
        scale = lambda a, b: float((a.float() - b.float()).detach().abs().max()) / max(float(b.float().detach().abs().max()), 1e-30)
        agree = {"max_output_diff_over_scale": max(scale(a, b) for a, b in zip(fo, eo)),
                 "max_gradient_diff_over_scale": max(scale(a, b) for a, b in zip(fg, eg))}

        # B: a third of the candidates unselected, a third of the gaussians filtered out
        opacity = rnd(n * K, 1)
        selection = torch.rand(n * K, device="cuda", generator=g) < 0.66
        M = int(selection.sum())
        radii = torch.randint(0, 3, (M,), device="cuda", generator=g, dtype=torch.int32)
        update_filter = radii > 0
        vgrad = rnd(M, 3)
        acc_f = [torch.zeros(N, 1, device="cuda"), torch.zeros(N, 1, device="cuda"), torch.zeros(N * K, 1, device="cuda"),
                 torch.zeros(N * K, 1, device="cuda")]
        acc_e = [a.clone() for a in acc_f]

        def fused_b():
            accumulate(*acc_f, idx, opacity, selection, radii, vgrad)

        def eager_b():
            eager_accumulate(acc_e, visible_mask, opacity, selection, update_filter, vgrad, K)

        fused_b()
        eager_b()
        torch.cuda.synchronize()
        agree["max_accumulator_diff_over_scale"] = max(scale(a, b) for a, b in zip(acc_f, acc_e))
        sides = {"fused_forward": forward_only(fused), "eager_forward": forward_only(eager),
                 "fused_forward_backward": step(fused), "eager_forward_backward": step(eager),
                 "fused_accumulate": fused_b, "eager_accumulate": eager_b}
        timed = time_alternating(list(sides.values()), args.iters, args.repeats, args.warmup)
        row = {name: {"ms": ms, "spread_ms": spread, "middle_half_spread_ms": iqr} for name, (ms, spread, iqr) in zip(sides, timed)}
        C = 3 + F + 3 * K + 6 + K                                   # floats per anchor row
        fwd = 4.0 * n * 2 * C + 9.0 * n                             # rows read and written once, idx, mask_anchor
        bwd = 4.0 * n * C + 4.0 * N * C + 4.0 * n * (6 + K) + 8.0 * n   # upstreams, dense gradients, grid_scaling, _mask, idx
        acc_b = 8.0 * n + 4.0 * n * K + 2.0 * n * K + 16.0 * n + M * (4.0 + 8.0) + 16.0 * M * 2 / 3
        # the eager side, each operand of each pass once: Quantize_anchor's 5 passes and exp / 1.0 * over N rows, the two
        # sigmoid chains (sigmoid, >, float, -, +) and the row sum over N K, then 6 masked gathers (mask + rows in and out)
        eager_fwd = 4.0 * N * (5 * 3 * 3 + 4 * 6) + 4.0 * N * K * (2 * 9.5 + 1) + 6.0 * N + 4.0 * n * 2 * C
        eager_bwd = eager_fwd + 4.0 * N * (C + 2 * C) + 4.0 * n * C + 4.0 * N * (3 * 6 + 3 * K)
        eager_acc = 4.0 * n * K * 6 + N * (2.0 + 16.0) + N * K * (1.0 * 6 + 16.0 * 2 / 3) + M * (1.0 + 12.0 + 8.0)
        share_of = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / rate, 4)
        row["algorithmic_mbytes"] = {
            "fused_forward": round(fwd / 1e6, 2), "fused_forward_backward": round((fwd + bwd) / 1e6, 2),
            "fused_accumulate": round(acc_b / 1e6, 2), "eager_forward": round(eager_fwd / 1e6, 2),
            "eager_forward_backward": round(eager_bwd / 1e6, 2), "eager_accumulate": round(eager_acc / 1e6, 2)}
        row["fused_share_of_copy_rate"] = {
            "forward": share_of(fwd, row["fused_forward"]["ms"]),
            "forward_backward": share_of(fwd + bwd, row["fused_forward_backward"]["ms"]),
            "accumulate": share_of(acc_b, row["fused_accumulate"]["ms"])}
        row["agreement_with_eager"] = agree
        for what in ("forward", "forward_backward", "accumulate"):
            row[f"eager_over_fused_{what}"] = round(row[f"eager_{what}"]["ms"] / row[f"fused_{what}"]["ms"], 2)
        result["visible"][str(share)] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
