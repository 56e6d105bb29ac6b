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


# ---------------------------------------------------------------- the sweep over the kernel's own regimes
REGIME_M = (0.0, 0.3, 1.0, 3.0, 4.5, 5.2, 6.0, 8.0, 13.0, 40.0, 1e3, 6e4, 7e4, 1e6, 1e9)     # and their negatives
NARROW = 0.25                                                                                # |d| <= NARROW: the series
REGIME_D = (0.0, 1e-8, 1e-4, 1e-2, 0.2, float(np.nextafter(np.float32(NARROW), np.float32(0))), NARROW,
            float(np.nextafter(np.float32(NARROW), np.float32(1))), 0.3, 1.0, 4.0, 30.0, 1e4,
            0.5)   # (0.5: where a series carried on past NARROW is furthest off, so that a moved threshold shows)
REGIME_SCALE = (0.0, -1.0, 5e-10, 1e-4, 0.3, 50.0)        # the first three reach the floor
REGIME_C = 2 * (len(REGIME_M) - 1) + 2                    # every signed m, and one column with |m| < d
REGIME_BLOCKS = 4
M_EDGES = (0.0, 1.0, 4.0, 6.0, float("inf"))
REGIONS = tuple((w, k) for w in ("narrow", "wide") for k in range(len(M_EDGES) - 1))


def kernel_d(q, scale):
    """d = q / 2s as the kernel forms it: fp32, the halving first."""
    s = np.maximum(np.asarray(scale, np.float32), np.float32(SCALE_FLOOR))
    return (np.float32(0.5) * np.asarray(q, np.float32)) / s


def _q_for(d, s):
    """the fp32 q whose kernel_d is the fp32 d where one exists (it is searched for the three values around NARROW),
    else the nearest"""
    q0 = np.float32(2.0 * float(s) * d)
    if not 0.2 < d < 0.3:
        return q0
    cand = [q0]
    for direction in (np.float32(0), np.float32(np.inf)):
        q = q0
        for _ in range(8):
            q = np.nextafter(q, direction)
            cand.append(q)
    cand = np.array(cand, np.float32)
    return cand[np.argmin(np.abs(kernel_d(cand, s).astype(np.float64) - d))]


def make_regime_inputs(seed):
    """Operands [n, REGIME_C] (fp32, CPU) that enter every branch of csrc/entropy.hip: row (block, d, scale) x column m.
    A row has one q = 2 s d (so q exists per row, per element, and -- for the rows sharing a value -- as one number); the
    columns are the signed REGIME_M, then m = d / 2 (|m| < d: the bin straddles the mean).  x_mean = 0 and x = 0 where
    the scale is at its floor (so that mean = -m s is not quantised by an ulp of x), else a few scales from 0: for a tiny
    or zero q the clamp collapses x onto x_mean -/+ 15000 q and c = that - mean.  mean is held within +-1e6, which caps
    |m| at 1e6 / s.  Block 0 is the lattice itself, 1 and 3 move m (3: d as well, except around NARROW) by up to 5 %, 2
    has q < 0 on every fifth row; three more rows make the last workgroup ragged.  What a check bins by is realised().
    -> dict x, mean, scale, q [n, 1], x_mean, g"""
    rng = np.random.RandomState(seed)
    ms = [s * m for m in REGIME_M[1:] for s in (1.0, -1.0)] + [0.0]
    rows = [(b, d, s) for b in range(REGIME_BLOCKS) for d in REGIME_D for s in REGIME_SCALE]
    rows += [(1, REGIME_D[i % len(REGIME_D)], REGIME_SCALE[(2 * i + 3) % len(REGIME_SCALE)]) for i in (4, 7, 11)]
    n = len(rows)
    x, mean = np.zeros((n, REGIME_C), np.float32), np.zeros((n, REGIME_C), np.float32)
    scale, q = np.zeros((n, REGIME_C), np.float32), np.zeros((n, 1), np.float32)
    for i, (b, d, sc) in enumerate(rows):
        s = max(np.float32(sc), np.float32(SCALE_FLOOR))
        if b == 3 and not 0.2 < d < 0.3:
            d = d * (1 + 0.05 * rng.uniform(-1, 1))
        q[i, 0] = _q_for(d, s) * (-1 if b == 2 and i % 5 == 0 else 1)
        scale[i] = sc
        m = np.array(ms + [0.5 * d * (1 if i % 2 else -1)])
        if b in (1, 3):
            m = m * (1 + 0.05 * rng.uniform(-1, 1, m.shape))
        x[i] = 0.0 if sc < 1e-9 else (float(s) * rng.uniform(-3, 3, REGIME_C)).astype(np.float32)
        span = np.float32(SPAN) * q[i, 0]
        xc = np.minimum(np.maximum(x[i], np.float32(0) - span), np.float32(0) + span)
        mean[i] = np.clip(xc.astype(np.float64) - m * float(s), -1e6, 1e6).astype(np.float32)
    g = rng.standard_normal((n, REGIME_C)).astype(np.float32)
    out = {"x": x, "mean": mean, "scale": scale, "q": q, "x_mean": np.zeros((), np.float32), "g": g}
    return {k: torch.from_numpy(v) for k, v in out.items()}


def realised(inp):
    """float64, from the fp32 operands after the clamp -> dict m, d, s, tu, tl, region (an index into REGIONS)"""
    i64 = {k: v.to(torch.float64) for k, v in inp.items()}
    lo, hi = clamp_bounds(i64["q"], i64["x_mean"], torch.float64)
    xc = torch.minimum(torch.maximum(i64["x"], lo), hi)
    s = torch.clamp(i64["scale"], min=SCALE_FLOOR)
    c, h = xc - i64["mean"], (0.5 * i64["q"]).expand_as(xc)
    m, d = c / s, h / s
    k = torch.bucketize(m.abs(), torch.tensor(M_EDGES[1:-1], dtype=torch.float64), right=True)
    region = torch.where(d.abs() <= NARROW, k, k + (len(M_EDGES) - 1))
    return {"m": m, "d": d, "s": s, "tu": (c + h) / s, "tl": (c - h) / s, "region": region}


def likelihood_from_the_tail(x, mean, scale, q, x_mean):
    """l of likelihood() from the side where neither cdf value is near 1 (the three forms of the header, no series):
    in float64 likelihood() itself is off by up to 2^-52 ABSOLUTE, which is all of an l below that."""
    lo, hi = clamp_bounds(q, x_mean, x.dtype)
    xc = torch.minimum(torch.maximum(x, lo), hi)
    s = torch.clamp(scale, min=SCALE_FLOOR)
    tu, tl = (xc + 0.5 * q - mean) / s, (xc - 0.5 * q - mean) / s
    a, b = torch.minimum(tu, tl) / math.sqrt(2), torch.maximum(tu, tl) / math.sqrt(2)
    return torch.where(a >= 0, 0.5 * (torch.erfc(a) - torch.erfc(b)),
                       torch.where(b <= 0, 0.5 * (torch.erfc(-b) - torch.erfc(-a)), 0.5 * (torch.erf(b) - torch.erf(a))))


MUTANTS = ("coefficient 1", "coefficient 2", "coefficient 3", "coefficient 4", "threshold 0.5", "threshold 0.01",
           "branch upper", "branch lower", "expm1")


def header_evaluation(x, mean, scale, q, x_mean, g, mutant=None):
    """include/bloomscene_entropy.h, sections HOW l IS COMPUTED and GRADIENT, operation by operation in the dtype of the
    operands (fp32 on the CPU: what the arithmetic of the header costs against float64, with libm's exp / erf / erfc /
    expm1 in place of the device library's): the branch selection, the five-term series with its guard, the expm1 forms
    of du - dl and tu du - tl dl, the gradient closed below the floor.  ``mutant`` (one of MUTANTS) breaks one piece.
    -> dict l, x, mean, scale, q (all [n, C]; q per element)"""
    assert mutant is None or mutant in MUTANTS
    lo, hi = clamp_bounds(q, x_mean, x.dtype)
    xc = torch.minimum(torch.maximum(x, lo), hi)
    s = torch.clamp(scale, min=SCALE_FLOOR)
    c, h = xc - mean, (0.5 * q).expand_as(x)
    tu, tl, m, d = (c + h) / s, (c - h) / s, c / s, h / s
    # the narrow bin
    coef = [1 / 6, 1 / 120, 1 / 5040, 1 / 362880]
    if mutant and mutant.startswith("coefficient"):
        k = int(mutant[-1]) - 1
        coef[k] = coef[k] * (100 if k == 3 else 10)
    u, d2 = m * m, d * d
    he2 = u - 1
    he4 = (u - 6) * u + 3
    he6 = ((u - 15) * u + 45) * u - 15
    he8 = (((u - 28) * u + 210) * u - 420) * u + 105
    series = 1 + d2 * (he2 * coef[0] + d2 * (he4 * coef[1] + d2 * (he6 * coef[2] + d2 * (he8 * coef[3]))))
    narrow = (2 * d) * (torch.exp(-0.5 * u) * 0.39894228040143267794) * series
    narrow = torch.where(u >= 256, d * 0, narrow)                       # the guard: exp(-u / 2) is 0 from u = 208 on
    # the wide bin
    k = 0.70710678118654752440
    up = tu >= tl
    a, b = torch.where(up, tl, tu) * k, torch.where(up, tu, tl) * k
    upper = 0.5 * (torch.erfc(a) - torch.erfc(b))
    lower = 0.5 * (torch.erfc(-b) - torch.erfc(-a))
    straddle = 0.5 * (torch.erf(b) - torch.erf(a))
    if mutant == "branch upper":
        upper = straddle
    if mutant == "branch lower":
        lower = straddle
    r = torch.where(a >= 0, upper, torch.where(b <= 0, lower, straddle))
    wide = torch.where(up, r, -r)
    D = torch.where(d.abs() <= (float(mutant[10:]) if mutant and mutant.startswith("threshold") else NARROW), narrow, wide)
    l = D.abs()
    # the gradient
    open_ = l >= FLOOR
    gl = torch.where(open_, -g / (l * 0.69314718055994530942), torch.zeros_like(l))
    ga = gl * torch.sign(D)
    inv = 0.39894228040143267794 / s
    du, dl = torch.exp(-0.5 * tu * tu) * inv, torch.exp(-0.5 * tl * tl) * inv
    qs = (q / s).expand_as(x)
    ex = m * qs
    expm1 = (lambda t: torch.exp(t) - 1) if mutant == "expm1" else torch.expm1
    neg = ex <= 0
    diff = torch.where(neg, -(du * expm1(ex)), dl * expm1(-ex))
    tdiff = torch.where(neg, tl * diff + qs * du, tu * diff + qs * dl)
    zero = torch.zeros_like(l)
    gd = torch.where(open_, ga * diff, zero)
    return {"l": l, "x": torch.where((x >= lo) & (x <= hi), gd, zero), "mean": -gd,
            "scale": torch.where((scale >= SCALE_FLOOR) & open_, -(ga * tdiff), zero),
            "q": torch.where(open_, ga * ((du + dl) * 0.5), zero)}


def regime_reference(inp):
    """float64 for the sweep -> dict l (likelihood), l_tail, x, mean, scale, q (autograd of gaussian_bits for inp["g"],
    q per element), scale_of (the yardstick of each gradient's error: its own magnitude; for scale
    |gl| (|tu| du + |tl| dl), whose two addends can cancel), real (realised())"""
    i64 = {k: v.to(torch.float64) for k, v in inp.items()}
    n, C = i64["x"].shape
    leaves = {k: i64[k].clone().requires_grad_(True) for k in ("x", "mean", "scale")}
    leaves["q"] = i64["q"].expand(n, C).clone().requires_grad_(True)
    gaussian_bits(leaves["x"], leaves["mean"], leaves["scale"], leaves["q"], i64["x_mean"]).backward(i64["g"])
    ref = {k: v.grad for k, v in leaves.items()}
    ref["l"] = likelihood(i64["x"], i64["mean"], i64["scale"], i64["q"], i64["x_mean"])
    ref["l_tail"] = likelihood_from_the_tail(i64["x"], i64["mean"], i64["scale"], i64["q"], i64["x_mean"])
    real = realised(inp)
    gl = torch.where(ref["l"] >= FLOOR, i64["g"].abs() / (ref["l"] * math.log(2)), torch.zeros_like(ref["l"]))
    phi = lambda t: torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi) / real["s"]
    # fp32 has steps of 2^-24 of a number only down to 2^-126: an exp(-t^2 / 2) below that (|t| > 13.2) comes in steps of
    # 2^-149 and goes into the gradient times |gl| / (s sqrt(2 pi)) (times max |t| for scale), so no yardstick is smaller
    small = 2.0 ** -126 * (1 + gl / (real["s"] * math.sqrt(2 * math.pi)))
    ref["scale_of"] = {"x": torch.maximum(ref["x"].abs(), small), "mean": torch.maximum(ref["mean"].abs(), small),
                       "q": torch.maximum(ref["q"].abs(), small),
                       "scale": torch.maximum(gl * (real["tu"].abs() * phi(real["tu"]) + real["tl"].abs() * phi(real["tl"])),
                                              small * torch.maximum(real["tu"].abs(), real["tl"].abs()).clamp(min=1))}
    ref["real"] = real
    return ref


UNIT = 2.0 ** -24


def regime_errors(got, ref, keep):
    """Per region the maximum error of ``got`` (dict l, x, mean, scale, q as float64 [n, C]) over the elements of ``keep``:
    l in units in the last place of the fp32 l64, each gradient in units of 2^-24 of ref["scale_of"] (0 / 0 counts as 0,
    anything else over 0 as inf; the gradient of scale only where the scale is not floored, as elsewhere it is 0 by rule).
    -> dict name -> list over REGIONS (None: no element)"""
    out = {}
    ulp = torch.from_numpy(np.spacing(ref["l"].numpy().astype(np.float32)).astype(np.float64))
    for name in ("l", "x", "mean", "scale", "q"):
        err = (got[name] - ref[name]).abs()
        unit = ulp if name == "l" else UNIT * ref["scale_of"][name]
        e = torch.where(err == 0, torch.zeros_like(err), err / unit)
        e = torch.where(torch.isnan(got[name]), torch.full_like(e, float("inf")), e)
        out[name] = []
        for k in range(len(REGIONS)):
            sel = keep & (ref["real"]["region"] == k)
            out[name].append(float(e[sel].max()) if sel.any() else None)
    return out


def regime_yardstick(inp, ref, mutant=None):
    """regime_errors of header_evaluation in fp32 on the CPU, over the elements at or above the floor and outside the band
    of 25 % around it"""
    got = header_evaluation(inp["x"], inp["mean"], inp["scale"], inp["q"], inp["x_mean"], inp["g"], mutant)
    keep = (ref["l"] >= FLOOR) & ((ref["l"] / FLOOR - 1).abs() > 0.25)
    return regime_errors({k: v.to(torch.float64) for k, v in got.items()}, ref, keep)


def regime_bar(figure):
    """The bar of the GPU test for one (quantity, region): twice the fp32 CPU figure -- the device library's exp and erfc
    round differently from libm's -- and never under 16 units, the accuracy OpenCL specifies for erf and erfc (to which
    the device library is written)."""
    return max(2.0 * figure, 16.0)
