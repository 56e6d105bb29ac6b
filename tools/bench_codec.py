"""Time the entropy codec (include/bloomscene_codec.h, bloomscene_amd/codec.py) at BloomScene's shape: 100 k anchors,
F = 50 features, 6 scalings and K = 10 offsets (three values each, 70 % of the offsets kept by the mask), the three
attribute streams of ``GaussianModel.conduct_encoding`` (scene/gaussian_model.py:1074-1214) for ALL anchors at once.

    python tools/bench_codec.py [--steps 10] [--warmup 2] [--anchors 100000]

Per stream and in total: the encode and the decode time (each call timed with events, host read included: the encoder's
call ends in the one read of its status and length; the median over ``steps`` after ``warmup`` calls), the stream's bits,
the ideal code length of the SAME integer model (``sum -log2((c(j + 1) - c(j)) / 65536)``, the header's ``c`` restated
here in torch with ``torch.exp`` in place of the pinned exp: a count of difference at most, nothing for a size), and
``entropy.rate_sum``'s estimate on the same operands.  Every decode is compared with ``rint(x / Q) * Q`` first.

THE EAGER SIDE IS NOT TIMED: the reference's path builds an ``[elements, L + 1]`` cdf table per batch of 1 000 anchors on
the GPU, copies it to the host and runs torchac's sequential CPU coder on it, and torchac is not installed on any machine
this project is built or tested on -- there is nothing to run.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bloomscene_amd import codec, entropy  # noqa: E402


def make_scene(n, F, K, seed):
    """A context matrix [n, 2 F + 12 + 6 K + 3] whose column blocks are the means and scales (read in place, strided),
    step sizes [n, 3] around BloomScene's 0.25, 2.5e-4 and 0.05, attributes drawn from the model and put on their steps,
    a 70 % offset mask."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    O = 2 * F + 12 + 6 * K + 3
    context = torch.zeros(n, O, device="cuda")
    Q = torch.tensor([0.25, 2.5e-4, 0.05], device="cuda") * (1 + 0.5 * torch.tanh(rn(n, 3)))
    xs, at = [], 0
    for c, (C, spread) in enumerate(((F, 1.0), (6, 0.2), (3 * K, 0.3))):
        unit = Q[:, c:c + 1].mean() * (4.0 if c != 1 else 200.0)          # scales of a few steps (hundreds for the scaling)
        mean = rn(n, C) * spread
        scale = rn(n, C).abs() * unit + 0.05 * unit
        context[:, at:at + C], context[:, at + C:at + 2 * C] = mean, scale
        x = mean + scale * rn(n, C)
        xs.append(torch.round(x / Q[:, c:c + 1]) * Q[:, c:c + 1])
        at += 2 * C
    masks = (torch.rand(n, K, 1, device="cuda", generator=g) < 0.7).float()
    return context, Q, xs[0], xs[1], xs[2].reshape(n, K, 3), masks


def phi(z):
    a = (z.abs() * 0.70710678118654752440).clamp(max=16.0)
    w = 0.3275911 * a
    u = w / (1.0 + w)
    p = -1.061405429 * u + 3.853875118
    for c in (-6.222859923, 5.874886615, -3.44449638, 1.0):
        p = p * u + c
    h = 0.5 * (p * torch.exp(-(a * a)))
    return torch.where(z < 0, h, 1.0 - h)


def ideal_bits(x, mean, scale, Q, keep, lo, L):
    """The code length of the header's integer model for the symbols of ``x`` (min ``lo``, ``L`` symbols)."""
    k = torch.round(x / Q)
    j = (k - lo).to(torch.int64)
    s = scale.clamp(min=1e-9)
    M = float(65536 - 2 * L)

    def c(j):
        z = (((j + lo).float() - 0.5) * Q - mean) / s
        inner = torch.round(phi(z) * M).to(torch.int64) + 2 * j
        return torch.where(j <= 0, torch.zeros_like(j), torch.where(j >= L, torch.full_like(j, 65536), inner))

    bits = -torch.log2((c(j + 1) - c(j)).double() / 65536.0)
    # (a skipped element's x is arbitrary and may lie outside [lo, lo + L): its term is not formed)
    return float(torch.where(keep != 0, bits, torch.zeros_like(bits)).sum()) if keep is not None else float(bits.sum())


def timed(fn, steps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--anchors", type=int, default=100_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_codec needs the GPU: there is no CPU path and no timing without one")
    n, F, K = args.anchors, 50, 10
    context, Q, feat, scaling, offsets, masks = make_scene(n, F, K, seed=0)
    mean, scale, mean_s, scale_s, mean_o, scale_o, _ = torch.split(context, [F, F, 6, 6, 3 * K, 3 * K, 3], dim=-1)
    keep = masks.reshape(n, K)
    blocks = {"feat": (feat, mean, scale, Q[:, 0:1], None, 1),
              "scaling": (scaling, mean_s, scale_s, Q[:, 1:2], None, 1),
              "offsets": (offsets.reshape(n, 3 * K), mean_o, scale_o, Q[:, 2:3], keep, 3)}
    out = {"anchors": n, "F": F, "K": K, "T": codec.DEFAULT_STEPS, "streams": {},
           "eager": "not timed: the reference's coder is torchac's CPU extension, which is not installed"}
    for name, (x, m, s, q, kp, r) in blocks.items():
        stream = codec.encode_gaussian(x, m, s, q, keep=kp, keep_repeat=r)
        y = codec.decode_gaussian(stream, m, s, q, keep=kp, keep_repeat=r)
        want = torch.round(x / q) * q
        if kp is not None:
            want = want * kp.repeat_interleave(r, dim=1)
        assert torch.equal(y, want), name
        header = stream[:32].cpu().numpy().view(np.int32)
        lo, L, chunks = int(header[4]), int(header[5]), int(header[7])
        coded = int(x.numel() if kp is None else kp.sum().item() * r)
        ideal = ideal_bits(x, m, s, q, None if kp is None else kp.repeat_interleave(r, dim=1), lo, L)
        estimate, _ = entropy.rate_sum(x, m, s, q, x.mean(), weight=kp, weight_repeat=r)
        enc_ms = timed(lambda: codec.encode_gaussian(x, m, s, q, keep=kp, keep_repeat=r), args.steps, args.warmup)
        dec_ms = timed(lambda: codec.decode_gaussian(stream, m, s, q, keep=kp, keep_repeat=r), args.steps, args.warmup)
        out["streams"][name] = {
            "elements": x.numel(), "coded": coded, "L": L, "chunks": chunks, "encode_ms": enc_ms, "decode_ms": dec_ms,
            "stream_bits": 8 * stream.numel(), "fixed_bits": 8 * (32 + 4 * (chunks + 1) + 256 * chunks), "ideal_bits": ideal,
            "rate_sum_bits": float(estimate), "stream_over_ideal": 8 * stream.numel() / ideal,
            "stream_over_rate_sum": 8 * stream.numel() / float(estimate),
            "encode_msym_per_s": coded / enc_ms / 1e3, "decode_msym_per_s": coded / dec_ms / 1e3}
    args_all = (context, Q, feat, scaling, offsets, masks, F, K)
    streams = codec.encode_attributes(*args_all)
    out["encode_ms"] = timed(lambda: codec.encode_attributes(*args_all), args.steps, args.warmup)
    out["decode_ms"] = timed(lambda: codec.decode_attributes(streams, context, Q, masks, F, K), args.steps, args.warmup)
    for key in ("stream_bits", "ideal_bits", "rate_sum_bits"):
        out[key] = sum(v[key] for v in out["streams"].values())
    out["stream_over_ideal"] = out["stream_bits"] / out["ideal_bits"]
    out["stream_over_rate_sum"] = out["stream_bits"] / out["rate_sum_bits"]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
