"""CPU restatements of the anchor heads (include/bloomscene_heads.h, bloomscene_amd/heads.py):

  (a) ``forward_np``     the header's function in numpy with a correctly rounded fp32 fma: X, pre1, hid, pre2 bit for bit
                         what the kernels compute (``fma32`` vectorised; ``fmaf_libm`` is libm's, to hold it against)
  (b) ``restatement``    gaussian_renderer/__init__.py:151-185 as eager BloomScene computes it (nn.functional.linear, relu,
                         tanh, sigmoid), generic in dtype, with an optional ``gate`` that replaces relu(pre1) by pre1 * gate
  (c) ``autograd64``     float64 autograd of (b) for given upstream gradients
  (d) ``scene``          seeded inputs: feat, anchor, a camera centre, the twelve weights, a 0/1 mask, upstreams
      ``backward_np64``  the header's analytic backward in numpy float64
      ``tanh_form`` / ``sigmoid_form``   the header's activation forms in fp32 numpy (bsr_expf restated)

THE SHARED GATE.  A hidden pre-activation within fp32 rounding of 0 takes the other ReLU branch in float64, which moves a
whole row's gradient by orders of magnitude; with n * 3 F hidden values a case that does happen.  So (b) and (c) are
evaluated with the gate of (a) -- which the GPU test pins bit for bit -- and all three differentiate the same
piecewise-linear function."""
import ctypes
import ctypes.util
from types import SimpleNamespace

import numpy as np
import torch

HEAD_OUTPUTS = (1, 7, 3)


# ---- (a) ----
def fma32(a, b, c):
    """round_fp32(a * b + c) exactly, elementwise: the product is exact in float64, TwoSum gives the sum's error, the sum
    is rounded to odd, and 53 >= 2 * 24 + 2 bits make the second rounding innocuous."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.uint64)
    inexact = np.isfinite(s) & (err != 0) & ((bits & np.uint64(1)) == 0)
    away = (err > 0) == (s > 0)          # the exact value lies beyond s in magnitude
    bits = np.where(inexact & away, bits + np.uint64(1), np.where(inexact & ~away, bits - np.uint64(1), bits))
    return bits.view(np.float64).astype(np.float32)


_libm = None


def fmaf_libm(a, b, c):
    """libm's fmaf through ctypes, one call per element (slow: for holding fma32 against)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fmaf.restype = ctypes.c_float
        _libm.fmaf.argtypes = [ctypes.c_float] * 3
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    out = np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())], np.float32)
    return out.reshape(a.shape)


def chain(X, W, b):
    """[n, J]: a = b[j]; for k ascending: a = fmaf(X[i, k], W[j, k], a)."""
    X, W = np.asarray(X, np.float32), np.asarray(W, np.float32)
    a = np.broadcast_to(np.asarray(b, np.float32)[None, :], (X.shape[0], W.shape[0])).copy()
    for k in range(W.shape[1]):
        a = fma32(X[:, k:k + 1], W[None, :, k], a)
    return a


def geometry_np(anchor, cam):
    anchor, cam = np.asarray(anchor, np.float32), np.asarray(cam, np.float32).reshape(3)
    d = anchor - cam[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
        v = (d / dist[:, None]).astype(np.float32)
    return v, dist


def forward_np(feat, anchor, cam, weights, K):
    """-> X [n, F + 4], pre1 [n, 3 F], hid [n, 3 F], pre2 [n, 11 K], gate [n, 3 F] (pre1 > 0), all fp32 as the header says."""
    feat = np.asarray(feat, np.float32)
    v, dist = geometry_np(anchor, cam)
    X = np.concatenate([feat, v, dist[:, None]], axis=1).astype(np.float32)
    pre1, hid, pre2 = [], [], []
    for h in range(3):
        W1, b1, W2, b2 = (np.asarray(w, np.float32) for w in weights[4 * h:4 * h + 4])
        p1 = chain(X, W1, b1)
        hh = np.where((p1 > 0) | np.isnan(p1), p1, np.float32(0)).astype(np.float32)
        pre1.append(p1)
        hid.append(hh)
        pre2.append(chain(hh, W2, b2))
    pre1, hid, pre2 = np.concatenate(pre1, 1), np.concatenate(hid, 1), np.concatenate(pre2, 1)
    return SimpleNamespace(X=X, pre1=pre1, hid=hid, pre2=pre2, gate=(pre1 > 0))


def _expf_form(x):
    """bsr_expf of csrc/common.h in numpy fp32 (finite, moderate arguments)."""
    x = np.asarray(x, np.float32)
    k = np.rint(x * np.float32(1.44269504088896341)).astype(np.float32)
    r = fma32(-k, np.float32(0.693359375), x)
    r = fma32(-k, np.float32(-2.12194440e-4), r)
    p = np.full_like(r, np.float32(1.0 / 5040.0))
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        p = fma32(p, r, np.float32(c))
    return np.ldexp(p, k.astype(np.int32)).astype(np.float32)


def tanh_form(x):
    x = np.asarray(x, np.float32)
    a = np.abs(x)
    u = a * a
    f = np.float32
    small = a * (f(1) + u * (f(-1.0 / 3.0) + u * (f(2.0 / 15.0) + u * (f(-17.0 / 315.0) + u * f(62.0 / 2835.0)))))
    e = _expf_form(f(-2) * a)
    big = (f(1) - e) / (f(1) + e)
    return np.copysign(np.where(a < f(0.25), small, big), x).astype(np.float32)


def sigmoid_form(x):
    x = np.asarray(x, np.float32)
    return (np.float32(1) / (np.float32(1) + _expf_form(-x))).astype(np.float32)


# ---- (b) ----
def restatement(feat, anchor, cam, weights, K, mask=None, gate=None):
    """GR:151-185 (use_feat_bank = False) -> (neural_opacity [n K, 1], color [n K, 3], scale_rot [n K, 7]).  ``gate`` [n, 3 F]
    (0 / 1): relu(pre1) becomes pre1 * gate."""
    n, F = feat.shape
    ob_view = anchor - cam.reshape(1, 3)                                       # GR:151
    ob_dist = ob_view.norm(dim=1, keepdim=True)                                # GR:153
    ob_view = ob_view / ob_dist                                                # GR:154
    cat = torch.cat([feat, ob_view, ob_dist], dim=1)                           # GR:168
    outs = []
    for h in range(3):
        W1, b1, W2, b2 = weights[4 * h:4 * h + 4]
        pre1 = torch.nn.functional.linear(cat, W1, b1)
        hid = torch.relu(pre1) if gate is None else pre1 * gate[:, h * F:(h + 1) * F].to(pre1.dtype)
        outs.append(torch.nn.functional.linear(hid, W2, b2))
    neural_opacity = torch.tanh(outs[0]).reshape(-1, 1)                        # GR:171
    if mask is not None:
        neural_opacity = neural_opacity * mask.reshape(-1, 1)                  # GR:172
    color = torch.sigmoid(outs[2]).reshape(n * K, 3)                           # GR:181
    scale_rot = outs[1].reshape(n * K, 7)                                      # GR:185
    return neural_opacity, color, scale_rot


# ---- (c) ----
def autograd64(feat, anchor, cam, weights, K, mask=None, ups=None, gate=None, heads=(0, 1, 2)):
    """float64 forward and autograd of (b).  ``ups`` = (g_opacity, g_color, g_scale_rot); ``heads``: whose outputs enter the
    backward (0 opacity, 1 cov, 2 color).  -> outputs and gradients as float64 numpy."""
    leaf = lambda t: t.detach().double().clone().requires_grad_(True)
    f, a = leaf(feat), leaf(anchor)
    m = None if mask is None else leaf(mask)
    w = [leaf(t) for t in weights]
    g = None if gate is None else torch.as_tensor(np.asarray(gate), dtype=torch.float64)
    opacity, color, scale_rot = restatement(f, a, cam.detach().double(), w, K, m, g)
    out = SimpleNamespace(opacity=opacity.detach().numpy(), color=color.detach().numpy(), scale_rot=scale_rot.detach().numpy())
    if ups is not None:
        terms = [(opacity, ups[0]), (scale_rot, ups[2]), (color, ups[1])]
        total = sum((terms[h][0] * terms[h][1].double()).sum() for h in heads)
        total.backward()
        z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
        out.d_feat, out.d_anchor = z(f), z(a)
        out.d_mask = None if m is None else z(m)
        out.d_weights = [z(t) for t in w]
    return out


def backward_np64(feat, anchor, cam, weights, K, mask, ups, gate):
    """The header's backward in float64 numpy (the forward quantities recomputed in float64 with the given gate)."""
    f8 = lambda t: np.asarray(t, np.float64)
    feat, anchor, cam = f8(feat), f8(anchor), f8(cam).reshape(3)
    n, F = feat.shape
    d = anchor - cam[None, :]
    dist = np.sqrt((d * d).sum(1))
    v = d / dist[:, None]
    X = np.concatenate([feat, v, dist[:, None]], 1)
    g_o, g_c, g_s = (f8(u).reshape(n, -1) for u in ups)
    m = np.ones((n, K)) if mask is None else f8(mask).reshape(n, K)
    dX = np.zeros_like(X)
    out = SimpleNamespace(d_weights=[])
    for h in range(3):
        W1, b1, W2, b2 = (f8(w) for w in weights[4 * h:4 * h + 4])
        gt = f8(gate)[:, h * F:(h + 1) * F]
        hid = (X @ W1.T + b1) * gt
        pre2 = hid @ W2.T + b2
        if h == 0:
            t = np.tanh(pre2)
            dpre2 = g_o * m * (1 - t * t)
            out.d_mask = g_o * t
        elif h == 1:
            dpre2 = g_s
        else:
            s = 1 / (1 + np.exp(-pre2))
            dpre2 = g_c * s * (1 - s)
        dpre1 = (dpre2 @ W2) * gt
        dX = dX + dpre1 @ W1
        out.d_weights += [dpre1.T @ X, dpre1.sum(0), dpre2.T @ hid, dpre2.sum(0)]
    gv, gd = dX[:, F:F + 3], dX[:, F + 3]
    s = (gv * v).sum(1)
    out.d_feat = dX[:, :F]
    out.d_anchor = (gv - v * s[:, None]) / dist[:, None] + gd[:, None] * v
    return out


# ---- (d) ----
def scene(n, F, K, seed=0, with_mask=True):
    """feat, anchor, cam, weights (nn.Linear's own scale), mask (0 / 1 with zeros), ups = (g_opacity, g_color, g_scale_rot)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * F + K)
    rn = lambda *s: torch.randn(*s, generator=g)
    weights = []
    for outputs in HEAD_OUTPUTS:
        for shape, fan in (((F, F + 4), F + 4), ((F,), F + 4), ((outputs * K, F), F), ((outputs * K,), F)):
            weights.append((torch.rand(*shape, generator=g) * 2 - 1) / fan ** 0.5)
    feat = rn(n, F)
    anchor = rn(n, 3) * 2.0
    cam = torch.tensor([0.3, -0.2, 4.0])
    mask = (torch.rand(n, K, 1, generator=g) < 0.7).float() if with_mask else None
    ups = (rn(n * K, 1), rn(n * K, 3), rn(n * K, 7))
    return SimpleNamespace(n=n, F=F, K=K, feat=feat, anchor=anchor, cam=cam, weights=weights, mask=mask, ups=ups)
