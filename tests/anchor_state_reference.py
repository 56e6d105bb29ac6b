"""CPU restatements of the anchor state (include/bloomscene_anchor_state.h, bloomscene_amd/anchor_state.py):

  (a) ``floor_div_np`` / ``quantize_anchor_np`` / ``visible_np``   the header's prologue in fp32 numpy, operation for
                         operation: what the kernels compute bit for bit (``heads_reference._expf_form`` / ``sigmoid_form``
                         are the library's exp and sigmoid)
  (b) ``eager_visible``  gaussian_renderer/__init__.py:34-46 over the model properties of scene/gaussian_model.py:342-364
                         and :394-399 as eager BloomScene computes them -- on ALL N rows, then the boolean-mask gathers --
                         generic in dtype and device (float64 for autograd)
  (c) ``mask_gradient64``  float64 autograd of (b)'s mask path
  (d) ``accumulate_np``  the header's epilogue in fp32 numpy;  ``eager_accumulate``  scene/gaussian_model.py:743-759 on
                         torch tensors
  (e) ``scene`` / ``epilogue_scene``   seeded inputs
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from heads_reference import _expf_form, sigmoid_form

LOGIT = math.log(0.01 / 0.99)       # sigmoid(LOGIT) = 0.01
BAND = 1e-4                         # no _mask input of a test lies within this of LOGIT
Q_ANCHOR = 1 / (2 ** 16 - 1)
SCAN_BLOCK = 1024                   # BSR_ANCHOR_STATE_SCAN
f32 = np.float32


# ---- (a) ----
def floor_div_np(a, b):
    """torch.div(a, b, rounding_mode='floor') on fp32, the header's sequence."""
    a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
    with np.errstate(all="ignore"):
        mod = np.fmod(a, b).astype(f32)
        div = ((a - mod) / b).astype(f32)
        div = np.where((mod != 0) & ((b < 0) != (mod < 0)), div - f32(1), div).astype(f32)
        q = np.floor(div).astype(f32)
        q = np.where(div - q > f32(0.5), q + f32(1), q).astype(f32)
        zero = np.copysign(f32(0), (a / b).astype(f32)).astype(f32)
        out = np.where(div != 0, q, zero)
        return np.where(b == 0, (a / b).astype(f32), out).astype(f32)


def quantize_anchor_np(anchor, bmin, bmax):
    anchor = np.asarray(anchor, f32)
    bmin, bmax = np.asarray(bmin, f32).reshape(1, 3), np.asarray(bmax, f32).reshape(1, 3)
    interval = ((bmax - bmin) * f32(Q_ANCHOR)).astype(f32) + f32(1e-6)
    q = floor_div_np(anchor - bmin, interval)
    q = np.where(q < 0, f32(0), np.where(q > 65535, f32(65535), q)).astype(f32)
    return ((q * interval).astype(f32) + bmin).astype(f32)


def visible_np(idx, anchor, bmin, bmax, feat, offset, scaling, mask):
    """-> anchor [n, 3], feat [n, F], grid_offsets [n, K, 3], grid_scaling [n, 6], binary_grid_masks [n, K, 1],
    mask_anchor [n] bool, mask_anchor_rate (fp32 scalar); a row whose index is outside [0, N) is zero."""
    idx = np.asarray(idx, np.int64)
    N = anchor.shape[0]
    ok = (idx >= 0) & (idx < N)
    r = np.where(ok, idx, 0)

    def rows(x):
        x = np.asarray(x, f32)[r]
        return np.where(ok.reshape((-1,) + (1,) * (x.ndim - 1)), x, f32(0)).astype(f32)

    K = offset.shape[1]
    a = quantize_anchor_np(np.asarray(anchor, f32)[r], bmin, bmax)
    a = np.where(ok[:, None], a, f32(0)).astype(f32)
    gs = np.where(ok[:, None], _expf_form(np.asarray(scaling, f32)[r]), f32(0)).astype(f32)
    s = sigmoid_form(np.asarray(mask, f32).reshape(N, K)[r])
    b = np.where(ok[:, None] & (s > f32(0.01)), f32(1), f32(0)).astype(f32)
    mask_anchor = b.max(axis=1, initial=0) > 0
    with np.errstate(all="ignore"):
        rate = f32(int(mask_anchor.sum())) / f32(idx.size)
    return a, rows(feat), rows(offset), gs, b.reshape(-1, K, 1), mask_anchor, f32(rate)


# ---- (b) ----
class _QuantizeAnchor(torch.autograd.Function):
    """utils/encodings.py:215-227: the quantised anchor forward, the upstream unchanged backward."""

    @staticmethod
    def forward(ctx, anchors, min_v, max_v):
        interval = (max_v - min_v) * Q_ANCHOR + 1e-6
        q = torch.clamp(torch.div(anchors - min_v, interval, rounding_mode="floor"), 0, 2 ** 16 - 1)
        return q * interval + min_v

    @staticmethod
    def backward(ctx, g):
        return g, None, None


def eager_visible(idx, anchor, bmin, bmax, feat, offset, scaling, mask):
    """The eager lines on torch tensors of any dtype / device; idx must be valid here."""
    N = anchor.shape[0]
    visible_mask = torch.zeros(N, dtype=torch.bool, device=anchor.device)
    visible_mask[idx] = True
    # get_anchor (Quantize_anchor, straight-through)
    get_anchor = _QuantizeAnchor.apply(anchor, bmin, bmax)
    get_scaling = 1.0 * torch.exp(scaling)
    sig = torch.sigmoid(mask)
    get_mask = ((sig > 0.01).to(sig.dtype) - sig).detach() + sig
    with torch.no_grad():
        get_mask_anchor = torch.sum(get_mask, dim=1)[:, 0] > 0
    mask_anchor = get_mask_anchor[visible_mask]
    rate = (mask_anchor.sum() / mask_anchor.numel()).detach()
    return (get_anchor[visible_mask], feat[visible_mask], offset[visible_mask], get_scaling[visible_mask],
            get_mask[visible_mask], mask_anchor.to(torch.bool), rate)


# ---- (c) ----
def mask_gradient64(idx, mask, g_masks):
    """d _mask [N, K, 1] in float64 by autograd of the eager mask path, for the upstream g_masks [n, K, 1]."""
    x = torch.as_tensor(np.asarray(mask, np.float64)).clone().requires_grad_(True)
    sig = torch.sigmoid(x)
    out = (((sig > 0.01).double() - sig).detach() + sig)[torch.as_tensor(np.asarray(idx, np.int64))]
    (out * torch.as_tensor(np.asarray(g_masks, np.float64))).sum().backward()
    return x.grad.numpy()


# ---- (d) ----
def accumulate_np(acc, idx, opacity, selection, filt, grad, K):
    """acc: the four accumulators (numpy fp32, flat); returns their updated copies.  filt: int32 radii or bool."""
    oa, ad, ga, od = (np.array(a, f32).reshape(-1).copy() for a in acc)
    idx = np.asarray(idx, np.int64)
    N, n, M = oa.size, idx.size, len(filt)
    o = np.asarray(opacity, f32).reshape(n, K)
    t = np.where(o < 0, f32(0), o).astype(f32)          # (a NaN stays)
    a = np.zeros(n, f32)
    for k in range(K):
        a = (a + t[:, k]).astype(f32)
    ok = (idx >= 0) & (idx < N)
    with np.errstate(invalid="ignore"):
        oa[idx[ok]] = (oa[idx[ok]] + a[ok]).astype(f32)
    ad[idx[ok]] = ad[idx[ok]] + f32(1)
    sel = np.asarray(selection).reshape(-1) != 0
    rank = np.cumsum(sel) - sel                          # exclusive, in candidate order
    keep = (np.asarray(filt) > 0) if np.asarray(filt).dtype != np.bool_ else np.asarray(filt)
    g = np.asarray(grad, f32).reshape(M, 3)
    norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(f32)).astype(f32)
    c = np.nonzero(sel)[0]
    j = rank[c]
    inside = j < M
    c, j = c[inside], j[inside]
    hit = keep[j] & ok[c // K]
    c, j = c[hit], j[hit]
    target = idx[c // K] * K + c % K
    ga[target] = (ga[target] + norm[j]).astype(f32)
    od[target] = od[target] + f32(1)
    return oa, ad, ga, od


def eager_accumulate(acc, idx, opacity, selection, update_filter, grad, K):
    """scene/gaussian_model.py:743-759 on clones of the four accumulators ([N, 1], [N, 1], [N K, 1], [N K, 1])."""
    opacity_accum, anchor_demon, offset_gradient_accum, offset_denom = (a.clone() for a in acc)
    anchor_visible_mask = torch.zeros(opacity_accum.shape[0], dtype=torch.bool, device=opacity_accum.device)
    anchor_visible_mask[idx] = True
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
    return opacity_accum, anchor_demon, offset_gradient_accum, offset_denom


# ---- (e) ----
def pick_idx(N, n, rng):
    """n strictly ascending rows of [0, N) that hold 0 and N - 1 where n allows."""
    if n == 0:
        return np.zeros(0, np.int64)
    if n == 1:
        return np.array([N - 1], np.int64)
    inner = rng.choice(np.arange(1, N - 1), size=n - 2, replace=False) if n > 2 else np.zeros(0, np.int64)
    return np.sort(np.concatenate([[0, N - 1], inner])).astype(np.int64)


def scene(N, F, K, n, seed=0):
    """Inputs of A: about half of the mask decisions 0, every seventh anchor with all K zero, no _mask within BAND of
    LOGIT (such a value is moved to the band's edge, not dropped); anchors below, inside and above the bounds; upstreams."""
    rng = np.random.default_rng(seed + 1000 * N + n)
    bmin = np.array([-1.5, -0.75, 0.25], f32)
    bmax = np.array([2.5, 1.25, 3.0], f32)
    anchor = (bmin + (bmax - bmin) * rng.uniform(-0.1, 1.1, (N, 3))).astype(f32)
    interval = ((bmax - bmin) * f32(Q_ANCHOR)).astype(f32) + f32(1e-6)
    exact = rng.integers(0, 65536, (N, 3)).astype(f32)
    anchor[::3] = ((exact * interval).astype(f32) + bmin)[::3]         # exact multiples q * interval + min
    feat = rng.standard_normal((N, F)).astype(f32)
    offset = rng.standard_normal((N, K, 3)).astype(f32)
    scaling = rng.uniform(-6, 1.5, (N, 6)).astype(f32)
    mask = (LOGIT + 2.0 * rng.standard_normal((N, K, 1))).astype(f32)
    mask[::7] = (LOGIT - 0.5 - np.abs(mask[::7] - LOGIT)).astype(f32)  # all K decisions 0
    near = np.abs(mask.astype(np.float64) - LOGIT) < BAND
    mask = np.where(near, np.where(mask >= LOGIT, LOGIT + 2 * BAND, LOGIT - 2 * BAND), mask).astype(f32)
    assert not (np.abs(mask.astype(np.float64) - LOGIT) < BAND).any()
    idx = pick_idx(N, n, rng)
    ups = [rng.standard_normal(s).astype(f32) for s in ((n, 3), (n, F), (n, K, 3), (n, 6), (n, K, 1))]
    return SimpleNamespace(N=N, F=F, K=K, n=n, idx=idx, anchor=anchor, bmin=bmin, bmax=bmax, feat=feat, offset=offset,
                           scaling=scaling, mask=mask, ups=ups)


def epilogue_scene(N, K, n, seed=0, M=None, padded=0, blocks=None, integer_norms=False, bool_filter=False):
    """Inputs of B on pre-filled accumulators.  blocks: per scan block "none" / "all" / anything else (random) for the
    selection mask; M: rows of radii / grad (default: the selected count); padded: rows appended with radius 0."""
    rng = np.random.default_rng(seed + 77 * N + n)
    idx = pick_idx(N, n, rng)
    opacity = rng.uniform(-1, 1, (n * K, 1)).astype(f32)
    selection = rng.random(n * K) < 0.6
    for b, kind in enumerate(blocks or ()):
        if kind in ("none", "all"):
            selection[b * SCAN_BLOCK:(b + 1) * SCAN_BLOCK] = kind == "all"
    count = int(selection.sum())
    M = (count if M is None else M) + padded
    radii = rng.integers(0, 3, M).astype(np.int32)       # a third are 0
    if padded:
        radii[M - padded:] = 0
    if integer_norms:
        triples = np.array([[3, 4], [6, 8], [5, 12], [8, 15], [0, 0], [-3, 4], [7, -24]], f32)
        xy = triples[rng.integers(0, len(triples), M)]
    else:
        xy = (rng.standard_normal((M, 2)) * 10.0 ** rng.uniform(-6, 2, (M, 1))).astype(f32)
    grad = np.concatenate([xy, rng.standard_normal((M, 1)).astype(f32)], axis=1).astype(f32)
    acc = [rng.integers(1, 9, (N, 1)).astype(f32) * f32(0.5), rng.integers(1, 9, (N, 1)).astype(f32),
           rng.integers(1, 9, (N * K, 1)).astype(f32) * f32(0.25), rng.integers(1, 9, (N * K, 1)).astype(f32)]
    filt = radii > 0 if bool_filter else radii
    return SimpleNamespace(N=N, K=K, n=n, M=M, idx=idx, opacity=opacity, selection=selection, radii=filt, grad=grad, acc=acc,
                           count=count)
