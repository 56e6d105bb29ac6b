"""The depth-prior regularisation of BloomScene's loss (bloomscene.py:298-325 over utils/loss.py:26-80,170-202), restated
twice for the tests of include/bloomscene_depth_loss.h:

  restatement(...)   dtype-generic torch, written from the formulas of the training loop (the two normalisations, HuberL1
                     with the image's edge weights, CMD with its moment loop, bilateral_filter through pad + unfold).  In
                     float64 with autograd it is the yardstick; in float32 on the GPU it is "the eager lines".
  evaluate(...)      numpy, the header's own formulas in the header's association: the maps r, o, h, b (in float32 they
                     are what the kernels compute; r, o, h hold no transcendental and are bit-equal) and the header's
                     ANALYTIC gradient.  (The scatter half A2 of the smoothness gradient is accumulated tap by tap, not in
                     the gather order of the header: a different rounding of the same sum.)

and the seeded scenes.  Nothing here touches the GPU by itself."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

SCENES = ("smooth", "noise", "rendered", "flat")
EDGE_SCENES = ("tied_M", "tied_wide", "near_flat")   # built for one branch each: scene() says which; not swept over every shape
SK_HEX = {0: "0x1.02d50cp-4", 1: "0x1.c8d656p-5", 2: "0x1.93285p-5", 4: "0x1.39fab6p-5", 5: "0x1.1515f8p-5",
          8: "0x1.7ce05p-6"}     # BSR_DEPTH_PRIOR_SK* of the header


# ---------------------------------------------------------------- torch: the training loop's lines
def normalise(depth):
    lo, hi = depth.min(), depth.max()
    return (depth - lo) / (hi - lo + 1e-8)


def huber_l1(pred, gt, rgb, tresh=0.2):
    """pred, gt [H, W]; rgb [H, W, 3] (any view)"""
    l1 = torch.abs(pred - gt)
    d = tresh * torch.max(l1)
    quad = ((pred - gt) ** 2 + d ** 2) / (2 * d)
    loss = torch.where(l1 >= d, l1, quad)
    gx = torch.mean(torch.abs(rgb[:, :-1, :] - rgb[:, 1:, :]), -1)
    gy = torch.mean(torch.abs(rgb[:-1, :, :] - rgb[1:, :, :]), -1)
    return (torch.exp(-gx) * loss[:, :-1]).mean() + (torch.exp(-gy) * loss[:-1, :]).mean()


def _matchnorm(a, b):
    power = torch.clamp(torch.pow(torch.abs(a - b) + 1e-6, 2), max=1e6)
    return torch.sqrt(torch.clamp(torch.sum(power), max=1e6) + 1e-6)


def cmd(x1, x2, n_moments=5):
    """x1, x2 [B, H, W]: the moment loop as written, for any batch"""
    x1 = torch.clamp(x1, min=-1e6, max=1e6)
    x2 = torch.clamp(x2, min=-1e6, max=1e6)
    m1, m2 = x1.mean(0), x2.mean(0)
    s1, s2 = x1 - m1, x2 - m2
    total = _matchnorm(m1, m2)
    for k in range(2, n_moments + 1):
        total = total + _matchnorm(torch.mean(torch.pow(torch.abs(s1) + 1e-6, k), 0),
                                   torch.mean(torch.pow(torch.abs(s2) + 1e-6, k), 0))
    return total / x1.shape[0]


def spatial_kernel(dtype=torch.float32, spatial_sigma=2.0, kernel_size=5):
    x = torch.arange(kernel_size, dtype=dtype) - kernel_size // 2
    y = x.unsqueeze(0).expand(kernel_size, kernel_size)
    k = torch.exp(-(y ** 2 + y.t() ** 2) / (2 * spatial_sigma ** 2))
    return k / k.sum()


def bilateral_map(depth, spatial_sigma=2.0, color_sigma=5.0, kernel_size=5):
    """depth [H, W] -> the per-pixel sum over the window, [H, W]"""
    H, W = depth.shape
    half = kernel_size // 2
    sk = spatial_kernel(depth.dtype, spatial_sigma, kernel_size).to(depth.device)
    padded = F.pad(depth[None, None], (half, half, half, half), mode="replicate")
    taps = F.unfold(padded, kernel_size=kernel_size).view(kernel_size, kernel_size, H, W).permute(2, 3, 0, 1)
    delta = depth[:, :, None, None] - taps
    colour = torch.exp(-delta.abs() / (2 * color_sigma ** 2))
    return torch.sum(sk * colour * delta ** 2, dim=(2, 3))


def bilateral(depth, spatial_sigma=2.0, color_sigma=5.0, kernel_size=5):
    return bilateral_map(depth, spatial_sigma, color_sigma, kernel_size).mean()


def restatement(D, P, rgb, value=None, domin=None, smooth=None, normalise_depths=True):
    """-> (loss, (Lv, Ld, Ls)); a term whose weight is None is 0"""
    r = normalise(D) if normalise_depths else D
    o = normalise(P) if normalise_depths else P
    zero = torch.zeros((), dtype=D.dtype, device=D.device)
    lv = huber_l1(r, o, rgb) if value is not None else zero
    ld = cmd(r[None], o[None]) if domin is not None else zero
    ls = bilateral(r) if smooth is not None else zero
    loss = zero
    for w, term in ((value, lv), (domin, ld), (smooth, ls)):
        if w is not None:
            loss = loss + w * term
    return loss, (lv, ld, ls)


def autograd64(D, P, rgb, value=None, domin=None, smooth=None, normalise_depths=True, upstream=1.0):
    """float64 on the CPU -> SimpleNamespace(out = [loss, Lv, Ld, Ls] as floats, grad [H, W] float64 numpy)"""
    leaf = D.double().clone().requires_grad_(True)
    loss, terms = restatement(leaf, P.double(), rgb.double(), value, domin, smooth, normalise_depths)
    (upstream * loss).backward()
    return SimpleNamespace(out=[loss.item()] + [t.item() for t in terms], grad=leaf.grad.numpy())


# ---------------------------------------------------------------- numpy: the header
def sk_table(dt):
    """[5, 5]: the header's constants in float32, the exact kernel in float64"""
    if dt == np.float32:
        return np.array([[float.fromhex(SK_HEX[i * i + j * j]) for j in range(-2, 3)] for i in range(-2, 3)], dtype=np.float32)
    return spatial_kernel(torch.float64).numpy()


def _sign(x):
    return np.sign(x).astype(x.dtype)


def evaluate(D, P, rgb, value=None, domin=None, smooth=None, normalise_depths=True, dt=np.float32, upstream=1.0):
    """D, P [H, W], rgb [H, W, 3] numpy.  -> SimpleNamespace(r, o, h, b maps; out = [loss, Lv, Ld, Ls] float64;
    G = dloss/dr; grad = dloss/dD times upstream; share_min, share_max, M, d, cnt_*)"""
    f = dt
    D, P, rgb = D.astype(f), P.astype(f), rgb.astype(f)
    H, W = D.shape
    HW = H * W
    tiny = f(1e-6)
    res = SimpleNamespace()
    with np.errstate(divide="ignore", invalid="ignore"):
        if normalise_depths:
            minD, maxD, minP, maxP = D.min(), D.max(), P.min(), P.max()
            rgD, rgP = (maxD - minD) + f(1e-8), (maxP - minP) + f(1e-8)
            r, o = (D - minD) / rgD, (P - minP) / rgP
        else:
            r, o = D, P
        sk = sk_table(f)
        # value
        e = r - o
        l1 = np.abs(e)
        M = l1.max()
        d = f(0.2) * M
        linear = l1 >= d
        h = np.where(linear, l1, (e * e + d * d) / (f(2) * d)).astype(f)
        ex, ey = np.zeros((H, W), f), np.zeros((H, W), f)
        if H >= 2 and W >= 2:
            ax = np.abs(rgb[:, :-1, :] - rgb[:, 1:, :])
            ay = np.abs(rgb[:-1, :, :] - rgb[1:, :, :])
            ex[:, :-1] = np.exp(-(((ax[..., 0] + ax[..., 1]) + ax[..., 2]) / f(3)))
            ey[:-1, :] = np.exp(-(((ay[..., 0] + ay[..., 1]) + ay[..., 2]) / f(3)))
        nx, ny = H * (W - 1), (H - 1) * W
        Lv = Ld = Ls = 0.0
        if value is not None:
            Lv = (ex * h).astype(np.float64).sum() / nx + (ey * h).astype(np.float64).sum() / ny
        # distribution
        cr, co = np.clip(r, f(-1e6), f(1e6)), np.clip(o, f(-1e6), f(1e6))
        ec = cr - co
        tt = np.abs(ec) + tiny
        pw = np.minimum(tt * tt, f(1e6))
        S = pw.astype(np.float64).sum()
        K = 4.0 * np.sqrt(HW * float(tiny) ** 2 + 1e-6)
        if domin is not None:
            Ld = np.sqrt(min(S, 1e6) + 1e-6) + K
        # smoothness
        pad = np.pad(r, 2, mode="edge")
        b = np.zeros((H, W), f)
        A1 = np.zeros((H, W), f)
        A2 = np.zeros((H, W), f)
        ys, xs = np.mgrid[0:H, 0:W]

        def slope(x):
            return np.exp(-(np.abs(x) / f(50))) * (f(2) * x - _sign(x) * ((x * x) / f(50)))

        for i in range(5):
            for j in range(5):
                delta = r - pad[i:i + H, j:j + W]
                b = b + (sk[i, j] * np.exp(-(np.abs(delta) / f(50)))) * (delta * delta)
                t1 = sk[i, j] * slope(delta)
                A1 = A1 + t1
                ny_, nx_ = np.clip(ys + i - 2, 0, H - 1), np.clip(xs + j - 2, 0, W - 1)
                np.add.at(A2, (ny_, nx_), t1)      # tap (i, j) of p lands on n(p, i, j)
        if smooth is not None:
            Ls = b.astype(np.float64).sum() / HW
        # gradient
        G = np.zeros((H, W), f)
        cnt_M = int((l1 == M).sum())
        if value is not None:
            a = ex / f(nx) + ey / f(ny)
            quad = ~linear
            Q = (a * (f(0.5) - (e * e) / (f(2) * (d * d))))[quad].astype(np.float64).sum()
            qM = f(float(f(0.2)) * Q / cnt_M) if f == np.float32 else 0.2 * Q / cnt_M
            Gv = np.where(linear, a * _sign(e), a * (e / d)).astype(f)
            Gv = np.where(l1 == M, Gv + _sign(e) * f(qM), Gv).astype(f)
            G = f(value) * Gv
        if domin is not None:
            sd = f(np.sqrt(min(S, 1e6) + 1e-6))
            gate = (S <= 1e6) & (np.abs(r) <= f(1e6)) & (tt * tt <= f(1e6))
            res.gate = gate
            Gd = np.where(gate, _sign(ec) * (tt / sd), f(0)).astype(f)
            G = G + f(domin) * Gd if value is not None else f(domin) * Gd
        if smooth is not None:
            Gs = (A1 - A2) / f(HW)
            G = G + f(smooth) * Gs if (value is not None or domin is not None) else f(smooth) * Gs
        G = G.astype(f)
        g = f(upstream)
        if normalise_depths:
            sG = G.astype(np.float64).sum()
            sGr = (G.astype(np.float64) * r.astype(np.float64)).sum()
            cnt_min, cnt_max = int((D == minD).sum()), int((D == maxD).sum())
            qmin = f((sGr - sG) / float(rgD) / cnt_min)
            qmax = f(-sGr / float(rgD) / cnt_max)
            grad = g * ((G / rgD + np.where(D == minD, qmin, f(0))) + np.where(D == maxD, qmax, f(0)))
            res.share_min, res.share_max, res.cnt_min, res.cnt_max = qmin, qmax, cnt_min, cnt_max
        else:
            grad = g * G
    loss = 0.0
    for w, term in ((value, Lv), (domin, Ld), (smooth, Ls)):
        if w is not None:
            loss = loss + float(f(w)) * term
    res.r, res.o, res.h, res.b = r.astype(f), o.astype(f), h, b.astype(f)
    res.out = [loss, Lv, Ld, Ls]
    res.G, res.grad = G, grad.astype(f)
    res.M, res.d, res.cnt_M, res.S, res.K = M, d, cnt_M, S, K
    res.l1 = l1
    return res


# ---------------------------------------------------------------- scenes
def tied_pixels(kind, H, W):
    """-> (neg, pos): flat indices of the pixels with e = -M and with e = +M, at least two pixels from every border and
    with disjoint 5 x 5 windows.  tied_M: 3 and 2.  tied_wide (80 x 80, four workgroups of 256 threads striding the
    6400 pixels in the linear reductions): 5 and 4, and (index // 256) % 4 takes all four values in either list, so every
    tie count has to be merged from four partials; the counts differ so that no two can be mistaken for each other."""
    if kind == "tied_wide":
        assert (H, W) == (80, 80)
        chosen = []
        for b, t in ((0, 1), (1, 2), (2, 3), (3, 5), (0, 3), (0, 5), (1, 3), (2, 1), (3, 0)):     # 256-pixel chunk 4 t + b
            chosen.append(next(at for at in range(256 * (4 * t + b) + 11 * len(chosen), 256 * (4 * t + b + 1))
                               if 2 <= at // W < H - 3 and 2 <= at % W < W - 3
                               and all(max(abs(at // W - c // W), abs(at % W - c % W)) >= 5 for c in chosen)))
        neg, pos = chosen[:5], chosen[5:]
    else:
        assert H >= 15 and W >= 15
        cells = [(H // 4, W // 4), (H // 4, 3 * W // 4), (H // 2, W // 2), (3 * H // 4, W // 4), (3 * H // 4, 3 * W // 4)]
        flat = [y * W + x for y, x in cells]
        neg, pos = flat[0::2], flat[1::2]
    for at in neg + pos:
        y, x = divmod(at, W)
        assert 2 <= y < H - 3 and 2 <= x < W - 3, (at, y, x)
    for a in neg + pos:
        for b in neg + pos:
            assert a == b or max(abs(a // W - b // W), abs(a % W - b % W)) >= 5, (a, b)
    return neg, pos


def clamp_gate_scene():
    """B3 of the clamp gates: -> (D, P) float32 [5, 5] for the distribution term alone without normalisation.  D lies
    beyond +-1e6 at three pixels, exactly at +1e6 and at -1e6 at one each; P is within 150 of the clamped D, so S < 1e6."""
    rng = np.random.RandomState(5)
    D = rng.uniform(-3, 3, (5, 5))
    D[0, 0], D[1, 2], D[4, 4], D[2, 2], D[3, 1] = 2e6, -5e6, 1.5e6, 1e6, -1e6
    P = np.clip(D, -1e6, 1e6) + rng.uniform(20, 150, (5, 5)) * rng.choice([-1.0, 1.0], (5, 5))
    return (torch.from_numpy(a.astype(np.float32)) for a in (D, P))


def scene(kind, H, W, seed=1):
    """-> (D, P, rgb): float32 torch tensors [H, W], [H, W], [H, W, 3].
    tied_M / tied_wide: D and P both span exactly [0, 4]; at the pixels tied_pixels() names D = 0, P = 4 (e = -o_max) or
    D = 4, P = 0 (e = +r_max), everywhere else both lie in [1, 3]: |r - o| (and |D - P|) is the SAME expression of the
    same values on all of them, bit-identical in any precision, and at most half of it elsewhere.  They are the tied
    minima and maxima of D and of P as well.  Around each, D is 2 on the 5 x 5 window and rgb one colour on the 2 x 2
    block: the pixels of one sign have one gradient, bit for bit.
    near_flat: D takes the four fp32 values 2 + k 2^-22, a range of three units of the value; P as in "smooth".
    smooth / noise / rendered: one pixel of P is raised well above the rest where D is lowest, so that the maximum of
    |r - o| (normalised or not) is unique and far from the runner-up in float32 and float64 alike.
    rendered: a block of exact zeros in D (the pixels a rasterizer leaves empty: tied minima) and two pixels sharing the
    maximum.  flat: D and P constant (M = 0: HuberL1's 0 / 0 branch exists and must never be selected)."""
    rng = np.random.RandomState(1000 * seed + 7 * H + W + 31 * (SCENES + EDGE_SCENES).index(kind))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = ys / max(H - 1, 1), xs / max(W - 1, 1)
    if kind in ("tied_M", "tied_wide"):
        D = 1.0 + 2.0 * rng.rand(H, W)
        P = 1.0 + 2.0 * rng.rand(H, W)
        rgb = rng.rand(H, W, 3)
        neg, pos = tied_pixels(kind, H, W)
        for at, (dv, pv) in [(a, (0.0, 4.0)) for a in neg] + [(a, (4.0, 0.0)) for a in pos]:
            y, x = divmod(at, W)
            D[y - 2:y + 3, x - 2:x + 3] = 2.0
            D[y, x], P[y, x] = dv, pv
            rgb[y:y + 2, x:x + 2] = 0.5
    elif kind == "near_flat":
        D = (np.float32(2.0) + np.float32(2.0 ** -22) * rng.randint(0, 4, (H, W)).astype(np.float32)).astype(np.float64)
        P = 1.5 + 0.9 * np.cos(2.5 * u - v) + 0.5 * v + 0.01 * rng.rand(H, W)
        rgb = rng.rand(H, W, 3)
        k = np.unravel_index(np.argmin(D), D.shape)
        P[D == D.max()] = P.max()
        P[k] = P.max() + 0.75 * (P.max() - P.min()) + 1.0
    elif kind == "flat":
        D = np.full((H, W), 1.75)
        P = np.full((H, W), 0.5)
        rgb = rng.rand(H, W, 3)
    else:
        if kind == "noise":
            D = 0.5 + 4.0 * rng.rand(H, W)
            P = 1.0 + 2.0 * rng.rand(H, W)
            rgb = rng.rand(H, W, 3)
        else:
            D = 2.0 + np.sin(3.0 * u + 0.5) * np.cos(2.0 * v) + 0.8 * u * v + 0.01 * rng.rand(H, W)
            P = 1.5 + 0.9 * np.cos(2.5 * u - v) + 0.5 * v + 0.01 * rng.rand(H, W)
            rgb = 0.5 + 0.4 * np.stack([np.sin(4 * u + v), np.cos(3 * v), np.sin(2 * u - 3 * v)], -1) + 0.02 * rng.rand(H, W, 3)
        if kind == "rendered":
            D[:max(1, H // 3), :max(1, W // 3)] = 0.0
            top = D.max() + 0.25
            D[H - 1, W - 1] = top
            D[0, W - 1] = top
        k = np.unravel_index(np.argmin(D), D.shape)      # (the first of the tied minima)
        P[D == D.max()] = P.max()                             # (r = 1 never meets o = 0: |r - o| = 1 at k alone)
        P[k] = P.max() + 0.75 * (P.max() - P.min()) + 1.0
    D, P, rgb = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (D, P, rgb))
    return D, P, rgb
