"""CPU restatements of the context head (include/bloomscene_context.h, bloomscene_amd/context.py), after
tests/heads_reference.py (whose correctly rounded ``fma32``, ``chain`` and ``tanh_form`` are used here):

  (a) ``forward_np``     the header's chains in numpy: pre1, hid, pre2 = context, the gate, adj, Q -- bit for bit what the
                         kernels compute
      ``steps_np`` / ``noised_np`` / ``quantise_np``   the step sizes, the training tail and the quantiser in np.float32,
                         in the header's source order (``quantise_np`` returns every intermediate)
  (b) ``restatement``    gaussian_renderer/__init__.py:76-97 ("GR") as eager BloomScene computes it, generic in dtype, the
                         caller's noise in place of randn_like, with an optional ``gate`` that replaces relu(pre1) by
                         pre1 * gate (THE SHARED GATE of heads_reference.py)
      ``restatement_quantise``   GR:133-142 with utils/encodings.py:196-212 (STE_multistep, use_clamp = True, tau = 1)
  (c) ``autograd64``     float64 autograd of (b) for given upstream gradients
  (d) ``scene``          seeded inputs: enc, the four weights, the attributes, noise, means, upstreams.  The last three
                         rows of W2 are scaled so that the adjustment columns spread over about +-3 (tanh takes both of
                         its branches, Q runs from 0.5 % to 200 % of q), and grid_scaling is log-normal around 0.4, so that
                         x / Q reaches thousands in the scaling column and the clamp at mean +- 15000 Q binds in rows
                         with a small Q, as in real scenes."""
from types import SimpleNamespace

import numpy as np
import torch

from heads_reference import chain, fma32, tanh_form  # noqa: F401  (fma32: for the tests)

Q_DEFAULT = (0.25, 2.5e-4, 5e-2)
f32 = np.float32


def outputs(F, K):
    return 2 * F + 12 + 6 * K + 3


def split_sizes(F, K):
    return [F, F, 6, 6, 3 * K, 3 * K, 1, 1, 1]      # GR:77-78


# ---- (a) ----
def steps_np(adj, q=Q_DEFAULT):
    """Q [n, 3] = q_c * (1 + tanh(adj_c))."""
    adj = np.asarray(adj, f32)
    return (np.asarray(q, f32)[None, :] * (f32(1) + tanh_form(adj))).astype(f32)


def forward_np(enc, weights, F, K, q=Q_DEFAULT):
    W1, b1, W2, b2 = (np.asarray(w, f32) for w in weights)
    pre1 = chain(np.asarray(enc, f32), W1, b1)
    hid = np.where((pre1 > 0) | np.isnan(pre1), pre1, f32(0)).astype(f32)
    pre2 = chain(hid, W2, b2)
    adj = pre2[:, -3:]
    return SimpleNamespace(pre1=pre1, hid=hid, pre2=pre2, gate=(pre1 > 0), adj=adj, Q=steps_np(adj, q))


def noised_np(x, noise, Qc):
    """x + noise * (Q + 1e-6f), [n, C] with Q [n]: three roundings in source order."""
    x, noise = np.asarray(x, f32), np.asarray(noise, f32)
    n = x.shape[0]
    sigma = (np.asarray(Qc, f32).reshape(n, 1) + f32(1e-6)).astype(f32)
    return (x.reshape(n, -1) + (noise.reshape(n, -1) * sigma).astype(f32)).astype(f32).reshape(x.shape)


def quantise_np(x, Qc, m):
    """STE_multistep of the header on x [n, C] with Q [n] and the mean m, every step in np.float32."""
    x = np.asarray(x, f32)
    n = x.shape[0]
    shape = x.shape
    x = x.reshape(n, -1)
    Q = np.asarray(Qc, f32).reshape(n, 1)
    m = f32(m)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lo = (m - (f32(15000) * Q).astype(f32)).astype(f32)
        hi = (m + (f32(15000) * Q).astype(f32)).astype(f32)
        xc = np.where(x < lo, lo, x).astype(f32)
        xc = np.where(xc > hi, hi, xc).astype(f32)
        ratio = (xc / Q).astype(f32)
        r = np.rint(ratio).astype(f32)
        Qq = (r * Q).astype(f32)
        d = (xc - Qq).astype(f32)
        out = (Qq + (tanh_form(d) * Q).astype(f32)).astype(f32)
        out64 = Qq.astype(np.float64) + np.tanh(d.astype(np.float64)) * Q.astype(np.float64)
    rs = lambda a: np.broadcast_to(a, x.shape).reshape(shape)
    return SimpleNamespace(lo=rs(lo), hi=rs(hi), clamped=rs(xc), ratio=rs(ratio), r=rs(r), Qq=rs(Qq), d=rs(d), out=rs(out),
                           out64=rs(out64), Q=rs(Q), bound=rs(xc != x))


# ---- (b) ----
def restatement(enc, weights, F, K, feat=None, grid_scaling=None, grid_offsets=None, noise=(None, None, None),
                q=Q_DEFAULT, gate=None):
    """GR:76-97 -> (feat_context [n, O], Q [n, 3], feat, grid_scaling, grid_offsets [n, K, 3]); ``noise`` holds what
    torch.randn_like drew at GR:91-93."""
    W1, b1, W2, b2 = weights
    pre1 = torch.nn.functional.linear(enc, W1, b1)
    hid = torch.relu(pre1) if gate is None else pre1 * gate.to(pre1.dtype)
    feat_context = torch.nn.functional.linear(hid, W2, b2)                                     # GR:76
    mean, scale, mean_scaling, scale_scaling, mean_offsets, scale_offsets, Q_feat_adj, Q_scaling_adj, Q_offsets_adj = \
        torch.split(feat_context, split_size_or_sections=split_sizes(F, K), dim=-1)           # GR:77-78
    Q_feat, Q_scaling, Q_offsets = q
    Q_feat = Q_feat * (1 + torch.tanh(Q_feat_adj))                                             # GR:82-84
    Q_scaling = Q_scaling * (1 + torch.tanh(Q_scaling_adj))
    Q_offsets = Q_offsets * (1 + torch.tanh(Q_offsets_adj))
    sigma_Q_feat = Q_feat + 1e-6                                                               # GR:87-89
    sigma_Q_scaling = Q_scaling + 1e-6
    sigma_Q_offsets = Q_offsets + 1e-6
    if feat is not None:
        noise_feat = noise[0] * sigma_Q_feat                                                   # GR:91
        feat = feat + noise_feat                                                               # GR:95
    if grid_scaling is not None:
        noise_grid_scaling = noise[1] * sigma_Q_scaling                                        # GR:92
        grid_scaling = grid_scaling + noise_grid_scaling                                       # GR:96
    if grid_offsets is not None:
        noise_grid_offsets = noise[2] * sigma_Q_offsets.unsqueeze(1)                           # GR:93
        grid_offsets = grid_offsets + noise_grid_offsets                                       # GR:97
    return feat_context, torch.cat([Q_feat, Q_scaling, Q_offsets], dim=1), feat, grid_scaling, grid_offsets


def ste_multistep(input, Q, input_mean, tau=1.0):
    """utils/encodings.py:198-209 with use_clamp = True."""
    input_min = input_mean - 15_000 * Q
    input_max = input_mean + 15_000 * Q
    input = torch.clamp(input, min=input_min.detach(), max=input_max.detach())
    Q_round = torch.round(input / Q)
    Q_q = Q_round * Q
    soft_part = torch.tanh((input - Q_q) / tau) * Q
    return Q_q + soft_part


def restatement_quantise(enc, weights, F, K, feat, grid_scaling, grid_offsets, means, q=Q_DEFAULT):
    """GR:133-142 -> (Q [n, 3], feat, grid_scaling, grid_offsets [n, K, 3])."""
    W1, b1, W2, b2 = weights
    feat_context = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(enc, W1, b1)), W2, b2)
    Q_feat_adj, Q_scaling_adj, Q_offsets_adj = torch.split(feat_context, split_size_or_sections=split_sizes(F, K), dim=-1)[-3:]
    Q_feat, Q_scaling, Q_offsets = q
    Q_feat = Q_feat * (1 + torch.tanh(Q_feat_adj))                                             # GR:137-139
    Q_scaling = Q_scaling * (1 + torch.tanh(Q_scaling_adj))
    Q_offsets = Q_offsets * (1 + torch.tanh(Q_offsets_adj))
    feat = ste_multistep(feat, Q_feat, means[0]).detach()                                      # GR:140-142
    grid_scaling = ste_multistep(grid_scaling, Q_scaling, means[1]).detach()
    grid_offsets = ste_multistep(grid_offsets, Q_offsets.unsqueeze(1), means[2]).detach()
    return torch.cat([Q_feat, Q_scaling, Q_offsets], dim=1), feat, grid_scaling, grid_offsets


# ---- (c) ----
GRAD_NAMES = ("d_enc", "d_feat", "d_scaling", "d_offsets", "d_W1", "d_b1", "d_W2", "d_b2")


def autograd64(s, gate=None, use=(0, 1, 2, 3, 4)):
    """float64 forward and autograd of (b) on the scene ``s``; ``use``: which of the five outputs (context, Q, feat,
    grid_scaling, grid_offsets) enter the backward with their upstream ``s.ups``.  -> outputs and gradients, float64 numpy."""
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    enc, feat, gs, go = leaf(s.enc), leaf(s.feat), leaf(s.grid_scaling), leaf(s.grid_offsets)
    w = [leaf(t) for t in s.weights]
    g = None if gate is None else torch.as_tensor(np.asarray(gate), dtype=torch.float64)
    outs = restatement(enc, w, s.F, s.K, feat, gs, go, [t.double() for t in s.noise], s.q, g)
    res = SimpleNamespace(outs=[o.detach().numpy() for o in outs])
    sum((outs[i] * s.ups[i].double()).sum() for i in use).backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    res.grads = [z(t) for t in (enc, feat, gs, go, *w)]
    return res


# ---- (d) ----
def scene(n, D, H, F, K, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 131 * D + 17 * F + K + 7 * H)
    rn = lambda *s: torch.randn(*s, generator=g)
    O = outputs(F, K)
    weights = [(torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5
               for shape, fan in (((H, D), D), ((H,), D), ((O, H), H), ((O,), H))]
    enc = rn(n, D) * 0.5
    # the adjustment columns: about +-3
    hid = torch.relu(enc.double() @ weights[0].double().T + weights[1].double())
    spread = (hid @ weights[2][-3:].double().T).abs().max() if n > 0 else torch.tensor(0.0)
    weights[2][-3:] *= float(3.0 / max(float(spread), 0.25))
    feat = rn(n, F)
    grid_scaling = torch.exp(rn(n, 6) * 0.8 - 1.0)
    grid_offsets = rn(n, K, 3) * 0.3
    noise = (rn(n, F), rn(n, 6), rn(n, K, 3))
    zero = torch.zeros(())
    means = tuple(t.mean() if n > 0 else zero for t in (feat, grid_scaling, grid_offsets))
    ups = (rn(n, O), rn(n, 3), rn(n, F), rn(n, 6), rn(n, K, 3))
    return SimpleNamespace(n=n, D=D, H=H, F=F, K=K, O=O, q=Q_DEFAULT, enc=enc, weights=weights, feat=feat,
                           grid_scaling=grid_scaling, grid_offsets=grid_offsets, noise=noise, means=means, ups=ups)
