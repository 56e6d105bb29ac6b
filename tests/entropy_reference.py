"""The rate term of BloomScene's loss restated in plain torch, in the dtype and on the device of its operands (float64 on
the CPU: the reference of the tests; float32 on the GPU: the numerics of the eager code the kernels replace).

"EM" is utils/entropy_models.py (Entropy_gaussian.forward :14-31, Low_bound :35-50), "GR" is
gaussian_renderer/__init__.py (:77-84 the split of the context, :100-127 the selection and the four rates).  The function
is the one include/bloomscene_entropy.h writes out.  One point of it is fixed in fp32 whatever the working dtype: the clamp
bounds ``x_mean -/+ 15000 q`` are DEFINED as the fp32 product and sum (they are detached constants of EM:20-22, and a
clamped x takes their value), so the float64 evaluation rounds them the same way before it goes on in float64.
"""
import math

import numpy as np
import torch

FLOOR = 1e-6        # EM:39
SCALE_FLOOR = 1e-9  # EM:23
SPAN = 15_000       # EM:20-21


def clamp_bounds(q, x_mean, dtype):
    """EM:20-21 in fp32 (the definition), handed on in ``dtype``."""
    q32, m32 = q.detach().to(torch.float32), x_mean.detach().to(torch.float32)
    span = SPAN * q32
    return (m32 - span).to(dtype), (m32 + span).to(dtype)


def _phi_cdf(v, mean, scale):
    """torch.distributions.Normal(mean, scale).cdf(v), the operations of EM:24-26 in their order."""
    return 0.5 * (1 + torch.erf((v - mean) * scale.reciprocal() / math.sqrt(2)))


def upper_lower(x, mean, scale, q, x_mean):
    """EM:20-26 -> (upper, lower, lo, hi)."""
    lo, hi = clamp_bounds(q, x_mean, x.dtype)
    xc = torch.minimum(torch.maximum(x, lo), hi)          # torch.clamp(x, min=lo, max=hi): lo > hi gives hi
    s = torch.clamp(scale, min=SCALE_FLOOR)
    return _phi_cdf(xc + 0.5 * q, mean, s), _phi_cdf(xc - 0.5 * q, mean, s), lo, hi


def likelihood(x, mean, scale, q, x_mean):
    """EM:27, before the floor."""
    upper, lower, _, _ = upper_lower(x, mean, scale, q, x_mean)
    return torch.abs(upper - lower)


class LowerBound(torch.autograd.Function):
    """EM:35-50 without its trip through the host: the forward floors at 1e-6, the backward passes g where the input was at
    least 1e-6 and nothing elsewhere (gate_literal below evaluates EM:43-50 word for word; test_entropy_cpu.py compares)."""

    @staticmethod
    def forward(ctx, l):
        ctx.save_for_backward(l)
        return torch.clamp(l, min=FLOOR)

    @staticmethod
    def backward(ctx, g):
        l, = ctx.saved_tensors
        return g * (l >= FLOOR).to(g.dtype)


def gate_literal(l, g):
    """EM:43-50 as written, on numpy arrays: zero g below the floor, then multiply by (l >= floor or g < 0)."""
    l, g = np.asarray(l), np.asarray(g)
    zeroed = g.copy()
    zeroed[l < FLOOR] = 0
    passes = np.logical_or(l >= FLOOR, g < 0.0)
    return zeroed * passes.astype(g.dtype)


def expand_weight(weight, r):
    """[n, C / r] -> [n, C]: column j takes weight[:, j // r] (GR:114: the [m, K, 1] mask .repeat(1, 1, 3).view(-1, 3 K))."""
    return weight.repeat_interleave(r, dim=1)


def gaussian_bits(x, mean, scale, q, x_mean, weight=None, r=1):
    """EM:14-31 (then GR:120 with a weight); differentiable by torch autograd."""
    bits = -torch.log2(LowerBound.apply(likelihood(x, mean, scale, q, x_mean)))
    return bits if weight is None else bits * expand_weight(weight, r)


def analytic_gradients(x, mean, scale, q, x_mean, g, weight=None, r=1):
    """The gradient formulas of the header for an upstream ``g [n, C]`` of the (weighted) bits, elementwise.
    -> dict x, mean, scale, q (all [n, C]: sum q over what it is broadcast over), weight ([n, C / r] or None)."""
    upper, lower, lo, hi = upper_lower(x, mean, scale, q, x_mean)
    l = torch.abs(upper - lower)
    bits = -torch.log2(torch.clamp(l, min=FLOOR))
    g_bits = g if weight is None else g * expand_weight(weight, r)
    gl = torch.where(l >= FLOOR, -g_bits / (l * math.log(2)), torch.zeros_like(l))
    sg = torch.sign(upper - lower)
    xc = torch.minimum(torch.maximum(x, lo), hi)
    s = torch.clamp(scale, min=SCALE_FLOOR)
    tu, tl = (xc + 0.5 * q - mean) / s, (xc - 0.5 * q - mean) / s
    du = torch.exp(-0.5 * tu * tu) / math.sqrt(2 * math.pi) / s
    dl = torch.exp(-0.5 * tl * tl) / math.sqrt(2 * math.pi) / s
    zero = torch.zeros_like(l)
    out = {
        "x": torch.where((x >= lo) & (x <= hi), gl * sg * (du - dl), zero),
        "mean": -gl * sg * (du - dl),
        "scale": torch.where(scale >= SCALE_FLOOR, -gl * sg * (tu * du - tl * dl), zero),
        "q": gl * sg * (du + dl) / 2,
        "weight": None,
    }
    if weight is not None:
        n, C = x.shape
        out["weight"] = (g * bits).reshape(n, C // r, r).sum(dim=2)
    return out


def rate_terms(feat, grid_scaling, grid_offsets, context, choose, grid_masks, mask_anchor_rate, feat_mean, scaling_mean,
               offsets_mean, feat_dim, n_offsets, q_feat=0.25, q_scaling=2.5e-4, q_offsets=5e-2):
    """GR:77-84 and GR:100-127 with their gathers -> (bit_per_param, bit_per_feat_param, bit_per_scaling_param,
    bit_per_offsets_param)."""
    mean, scale, mean_s, scale_s, mean_o, scale_o, adj_f, adj_s, adj_o = torch.split(
        context, [feat_dim, feat_dim, 6, 6, 3 * n_offsets, 3 * n_offsets, 1, 1, 1], dim=-1)
    Qf = q_feat * (1 + torch.tanh(adj_f))
    Qs = q_scaling * (1 + torch.tanh(adj_s))
    Qo = q_offsets * (1 + torch.tanh(adj_o))
    c = choose
    masks = grid_masks[c].repeat(1, 1, 3).view(-1, 3 * n_offsets)
    bit_feat = gaussian_bits(feat[c], mean[c], scale[c], Qf[c], feat_mean)
    bit_scaling = gaussian_bits(grid_scaling[c], mean_s[c], scale_s[c], Qs[c], scaling_mean)
    bit_offsets = gaussian_bits(grid_offsets[c].view(-1, 3 * n_offsets), mean_o[c], scale_o[c], Qo[c], offsets_mean) * masks
    per_feat = torch.sum(bit_feat) / bit_feat.numel() * mask_anchor_rate
    per_scaling = torch.sum(bit_scaling) / bit_scaling.numel() * mask_anchor_rate
    per_offsets = torch.sum(bit_offsets) / bit_offsets.numel() * mask_anchor_rate
    per_param = (torch.sum(bit_feat) + torch.sum(bit_scaling) + torch.sum(bit_offsets)) / \
        (bit_feat.numel() + bit_scaling.numel() + bit_offsets.numel()) * mask_anchor_rate
    return per_param, per_feat, per_scaling, per_offsets


def make_inputs(n, C, seed, q_kind="row"):
    """The test inputs (fp32, CPU): mean ~ N(0, 1), scale = 0.3 exp(N(0, 1)), x = mean + N(0, 1) scale k with k = 6 on a
    fifth of the elements (about 7.5 % of the likelihoods at the floor), q = 0.25 (1 + tanh N(0, 1)) + 1e-6 as one value
    ("single"), per row ("row") or per element ("element"); a few elements beyond either clamp bound with the mean next to
    the bound, a few scales below 1e-9 (one of them with x on the mean).  -> dict x, mean, scale, q, x_mean, g."""
    gen = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(tuple(shape), generator=gen, dtype=torch.float64)

    mean = randn(n, C)
    scale = 0.3 * torch.exp(randn(n, C))
    k = torch.where(torch.rand(n, C, generator=gen) < 0.2, 6.0, 1.0).to(torch.float64)
    x = mean + randn(n, C) * scale * k
    q_shape = {"single": (), "row": (n, 1), "element": (n, C)}[q_kind]
    q = (0.25 * (1 + torch.tanh(randn(*q_shape))) + 1e-6).to(torch.float32)
    x, mean, scale = x.to(torch.float32), mean.to(torch.float32), scale.to(torch.float32)
    x_mean = x.mean() if x.numel() else torch.zeros(())
    total = n * C
    if total >= 12:
        lo, hi = clamp_bounds(q, x_mean, torch.float32)
        lo, hi = lo.expand(n, C).reshape(-1), hi.expand(n, C).reshape(-1)
        pick = torch.randperm(total, generator=gen)[:8]
        xf, mf, sf = x.view(-1), mean.view(-1), scale.view(-1)
        for t, e in enumerate(pick[:4].tolist()):            # beyond a clamp bound, the mean within a scale of the bound
            bound = hi[e] if t % 2 == 0 else lo[e]
            xf[e] = bound + (1.0 + abs(float(bound))) * (0.5 if t % 2 == 0 else -0.5)
            mf[e] = bound + 0.3 * sf[e]
        for t, e in enumerate(pick[4:].tolist()):            # scales below the floor: 0, negative, tiny
            sf[e] = (0.0, -1.0, 1e-10, 5e-10)[t]
        xf[pick[4]] = mf[pick[4]]
    g = torch.randn(n, C, generator=gen, dtype=torch.float64).to(torch.float32)
    return {"x": x, "mean": mean, "scale": scale, "q": q, "x_mean": x_mean.to(torch.float32), "g": g}
