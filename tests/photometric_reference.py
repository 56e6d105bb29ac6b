"""The photometric loss of include/bloomscene_loss.h restated in numpy, one array operation per stated operation (numpy
rounds every operation by itself, so fp32 stays uncontracted), in the association the header fixes.  ``dtype`` float32 is
what the kernels must reproduce bit for bit; float64 is compared with the formula of utils/loss.py.  Also the scenes the
tests share and exact sums (``math.fsum``) of the elementwise terms."""
import math
from types import SimpleNamespace

import numpy as np
import torch

WINDOW_HEX = ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2")
SCENES = ("noise", "smooth", "flat", "hdr")


def window(dtype=np.float32):
    """w[0..10]: the header's six constants, mirrored."""
    half = [float.fromhex(h) for h in WINDOW_HEX]
    return np.array(half + half[-2::-1], dtype=dtype)


def _pass(t, w, axis):
    """acc = 0; acc = acc + w[k] * t[.. + k - 5], zeros outside, along one axis."""
    n = t.shape[axis]
    shape = list(t.shape)
    shape[axis] = n + 10
    padded = np.zeros(shape, dtype=t.dtype)
    at = [slice(None)] * t.ndim
    at[axis] = slice(5, 5 + n)
    padded[tuple(at)] = t
    acc = np.zeros_like(t)
    for k in range(11):
        at[axis] = slice(k, k + n)
        acc = acc + w[k] * padded[tuple(at)]
    return acc


def conv(t, w):
    """Rows first, then columns; t is [..., H, W]."""
    return _pass(_pass(t, w, t.ndim - 1), w, t.ndim - 2)


def evaluate(img, gt, lam, dtype=np.float32, g=1.0):
    """img, gt [B, C, H, W] arrays -> map, partials (pMu, pE11, pE12), abs_diff, out = (loss, L1, S) from exact sums of the
    elements (python floats: the kernels' fp32 results are compared with these within one unit), grad for the upstream g."""
    img, gt = np.asarray(img, dtype=dtype), np.asarray(gt, dtype=dtype)
    w = window(dtype)
    two, one = dtype(2), dtype(1)
    C1, C2 = dtype(1e-4), dtype(9e-4)
    lam = dtype(lam)
    N = img.size
    mu1, mu2 = conv(img, w), conv(gt, w)
    e11, e22, e12 = conv(img * img, w), conv(gt * gt, w), conv(img * gt, w)
    p12, q1, q2 = mu1 * mu2, mu1 * mu1, mu2 * mu2
    s1, s2, s12 = e11 - q1, e22 - q2, e12 - p12
    a, b = two * p12 + C1, two * s12 + C2
    c, d = (q1 + q2) + C1, (s1 + s2) + C2
    ab, cd = a * b, c * d
    m = ab / cd
    p_mu = ((two * mu2) * (b - a)) / cd - (((two * mu1) * ab) * (d - c)) / (cd * cd)
    p_e11 = -(ab / (cd * d))
    p_e12 = (two * a) / cd
    diff = img - gt
    abs_diff = np.abs(diff)
    r = SimpleNamespace(map=m, partials=(p_mu, p_e11, p_e12), abs_diff=abs_diff)
    if N:
        l1 = math.fsum(abs_diff.ravel().tolist()) / N
        s = math.fsum(m.ravel().tolist()) / N
        r.out = ((1.0 - float(lam)) * l1 + float(lam) * (1.0 - s), l1, s)
    else:
        r.out = (0.0, 0.0, 0.0)
    n = dtype(N)
    kl, ks = (one - lam) / n, -lam / n
    sg = np.sign(diff)
    inner = (conv(p_mu, w) + (two * img) * conv(p_e11, w)) + gt * conv(p_e12, w)
    r.grad_unit = kl * sg + ks * inner            # what the upstream multiplies
    r.grad = dtype(g) * r.grad_unit
    return r


def scene(kind, B, C, H, W, seed=1):
    """-> (img, gt) float32 [B, C, H, W] torch tensors on the CPU.
    noise: two independent uniform images.  smooth: gt = 0.5 + 0.4 sin(7x + 3y), 0.5 + 0.4 cos(5y), x y (by channel % 3) on
    the unit square, img = clamp(gt + 0.03 randn).  flat: gt = 0.9, img = gt + 1e-3 randn in the lower half, = gt above.
    hdr: an unclamped render against a target in [0, 1]: gt uniform, img = gt + 1.5 randn held to [-2, 6]; nothing in the
    formula or the kernels assumes [0, 1]."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand(B, C, H, W, generator=gen), torch.rand(B, C, H, W, generator=gen)
    if kind == "smooth":
        y = torch.linspace(0, 1, H).view(H, 1).expand(H, W)
        x = torch.linspace(0, 1, W).view(1, W).expand(H, W)
        planes = (0.5 + 0.4 * torch.sin(7 * x + 3 * y), 0.5 + 0.4 * torch.cos(5 * y), x * y)
        gt = torch.stack([planes[ch % 3] for ch in range(C)]).expand(B, C, H, W).contiguous()
        return (gt + 0.03 * torch.randn(B, C, H, W, generator=gen)).clamp(0, 1), gt
    if kind == "flat":
        gt = torch.full((B, C, H, W), 0.9)
        img = gt + 1e-3 * torch.randn(B, C, H, W, generator=gen)
        img[:, :, :H // 2] = gt[:, :, :H // 2]
        return img, gt
    if kind == "hdr":
        gt = torch.rand(B, C, H, W, generator=gen)
        return (gt + 1.5 * torch.randn(B, C, H, W, generator=gen)).clamp(-2, 6), gt
    raise ValueError(kind)
