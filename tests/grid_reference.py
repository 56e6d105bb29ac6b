"""CPU restatement of the hash-grid encoder of include/bloomscene_grid.h (test infrastructure).

numpy, fp32, vectorised over points, looping over levels and corners in the kernels' order with elementwise operations
only (np.sum is pairwise: every sequential sum here is written out).  The GPU forward is bit-equal to `forward`, the
GPU backward to `backward` (the int64 fixed-point rule: np.add.at on int64 is exact).  `forward_f64` is an independent
float64 torch twin of the interpolation that pins the restatement itself.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
PRIMES = (1, 2654435761, 805459861)


def _level(offsets, resolutions, l):
    off = int(offsets[l])
    hs = (int(offsets[l + 1]) - off) & 0xFFFFFFFF
    res = int(resolutions[l]) & 0xFFFFFFFF
    return off, hs, res


def _rows(p, hs, res):
    """Row (relative to the level) of the grid points p [n, D] uint32: dense while the stride fits, else hashed."""
    D = p.shape[1]
    stride, index, d = 1, np.zeros(p.shape[0], np.uint32), 0
    while d < D and stride <= hs:
        index = index + p[:, d] * np.uint32(stride)
        stride = (stride * res) & 0xFFFFFFFF
        d += 1
    if stride > hs:
        index = np.zeros(p.shape[0], np.uint32)
        for d in range(D):
            index = index ^ (p[:, d] * np.uint32(PRIMES[d]))
    return index % np.uint32(hs)


def pos_fused(x, res):
    """x * float(res - 2) + 0.5 rounded ONCE to fp32: what a contracting compiler's v_fma_f32 gives (the reference's double
    0.5 narrows to fp32 without moving a bit, then fuses).  Exact: the product of two fp32 is exact in float64; the sum
    is rounded to odd in float64 (TwoSum residual), and 53 >= 24 + 2 bits make the final rounding to fp32 a single one."""
    p = np.asarray(x, F32).astype(np.float64) * float((int(res) - 2) & 0xFFFFFFFF)
    s = p + 0.5
    bb = s - p
    e = (p - (s - bb)) + (0.5 - bb)                      # exact residual of the float64 sum
    toward = np.where(e > 0, np.inf, -np.inf)
    other = np.nextafter(s, toward)
    odd = (s.view(np.int64) & 1) == 1
    s = np.where((e != 0) & ~odd, other, s)
    return s.astype(F32)


def _cell(x, hs, res, rows_left, pos=None):
    """pos, per-corner weights, inclusion, rows and wn_re of every point (x [N, D] fp32, inside [0, 1]).  pos: the
    position before floor() if it is not the specification's x * scale + 0.5 in fp32 (pos_fused)."""
    N, D = x.shape
    scale = F32(float((res - 2) & 0xFFFFFFFF))
    pos = x * scale + F32(0.5) if pos is None else np.ascontiguousarray(pos, F32)
    pg = np.floor(pos).astype(np.uint32)
    pos = pos - pg.astype(F32)
    ws, oks, rows = [], [], []
    wn = np.zeros(N, F32)
    for k in range(1 << D):
        w = np.ones(N, F32)
        p = np.empty((N, D), np.uint32)
        ok = np.ones(N, bool)
        for d in range(D):
            if (k >> d) & 1 == 0:
                w = w * (F32(1) - pos[:, d])
                p[:, d] = pg[:, d]
            else:
                w = w * pos[:, d]
                p[:, d] = np.minimum(pg[:, d] + np.uint32(1), np.uint32((res - 1) & 0xFFFFFFFF))
            ok &= (p[:, d] != 0) & (p[:, d] != np.uint32((res - 1) & 0xFFFFFFFF))
        ok &= hs != 0
        row = _rows(p, hs, res) if hs != 0 else np.zeros(N, np.uint32)
        ok &= row.astype(np.int64) < rows_left
        row = np.where(ok, row, 0)
        wn = np.where(ok, wn + w, wn)
        ws.append(w), oks.append(ok), rows.append(row)
    wn = np.where(wn == 0, F32(1e-9), wn)
    wn_re = F32(1) / wn
    return pos, ws, oks, rows, wn_re


def _inside(x):
    return np.all((x >= 0) & (x <= 1), axis=1)


def forward(inputs, embeddings, offsets, resolutions, n_levels=None, with_dy_dx=True):
    """-> outputs [L, N, F] fp32, dy_dx [N, L, D, F] fp32 (or None).  offsets / resolutions: the computed levels'
    (already sliced) lists; embeddings: the whole table."""
    x = np.ascontiguousarray(inputs, F32)
    emb = np.ascontiguousarray(embeddings, F32)
    N, D = x.shape
    R, F = emb.shape
    L = len(resolutions) if n_levels is None else n_levels
    out = np.zeros((L, N, F), F32)
    dy = np.zeros((N, L, D, F), F32) if with_dy_dx else None
    inside = _inside(x)
    xi = x[inside]
    for l in range(L):
        off, hs, res = _level(offsets, resolutions, l)
        pos, ws, oks, rows, wn_re = _cell(xi, hs, res, R - off)
        val = [np.where(ok[:, None], emb[np.clip(off + row.astype(np.int64), 0, max(R - 1, 0))], F32(0))
               for ok, row in zip(oks, rows)]
        o = np.zeros((xi.shape[0], F), F32)
        for k in range(1 << D):
            o = np.where(oks[k][:, None], o + (ws[k] * wn_re)[:, None] * val[k], o)
        out[l, inside] = o
        if with_dy_dx:
            scale = F32(float((res - 2) & 0xFFFFFFFF))
            for gd in range(D):
                rg = np.zeros((xi.shape[0], F), F32)
                for idx in range(1 << (D - 1)):
                    w = np.full(xi.shape[0], scale, F32)
                    corner = 0
                    for nd in range(D - 1):
                        d = nd + 1 if nd >= gd else nd
                        if (idx >> nd) & 1 == 0:
                            w = w * (F32(1) - pos[:, d])
                        else:
                            w = w * pos[:, d]
                            corner |= 1 << d
                    rg = rg + w[:, None] * (val[corner | (1 << gd)] - val[corner])
                dy[inside, l, gd] = rg
    return out, dy


def _exponent(gbits):
    """e with G < 2^e (frexp) of a non-zero finite |G| given by its bits."""
    E = gbits >> 23
    if E:
        return E - 126
    return int(gbits & 0x7FFFFF).bit_length() - 149


def scale_exp(gmax_bits, N, D):
    """s_l of the header."""
    if gmax_bits == 0:
        return 0
    k = (int(N - 1).bit_length() if N > 1 else 0) + D
    return min(61 - k - _exponent(int(gmax_bits)), 126)


def level_gmax_bits(grad_l):
    a = np.ascontiguousarray(grad_l, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    a = a[a < 0x7F800000]
    return int(a.max()) if a.size else 0


def contributions(inputs, offsets, resolutions, n_rows, grad, n_levels=None):
    """Per level: (element index (row * F + ch) [M], v fp32 [M]) of every contribution, in no particular order."""
    x = np.ascontiguousarray(inputs, F32)
    g = np.ascontiguousarray(grad, F32)
    L, N, F = g.shape
    D = x.shape[1]
    inside = _inside(x)
    xi = x[inside]
    per_level = []
    for l in range(L):
        off, hs, res = _level(offsets, resolutions, l)
        pos, ws, oks, rows, wn_re = _cell(xi, hs, res, n_rows - off)
        gl = g[l, inside]
        idx, vals = [], []
        for k in range(1 << D):
            ww = ws[k] * wn_re
            v = ww[:, None] * gl
            e = (off + rows[k].astype(np.int64))[:, None] * F + np.arange(F)[None, :]
            idx.append(e[oks[k]].ravel()), vals.append(v[oks[k]].ravel())
        per_level.append((np.concatenate(idx), np.concatenate(vals).astype(F32)))
    return per_level


def backward(inputs, offsets, resolutions, n_rows, grad, dy_dx=None):
    """-> grad_embeddings [n_rows, F] (the fixed-point rule of the header), grad_inputs [N, D] (or None), and the
    per-level scale exponents s_l.  grad [L, N, F]; dy_dx [N, L, D, F] from `forward`."""
    g = np.ascontiguousarray(grad, F32)
    L, N, F = g.shape
    D = np.asarray(inputs).shape[1]
    acc = np.zeros(n_rows * F, np.int64)
    bad = np.zeros(n_rows * F, bool)
    out = np.zeros(n_rows * F, F32)
    s_all = []
    for l, (e, v) in enumerate(contributions(inputs, offsets, resolutions, n_rows, g)):
        s = scale_exp(level_gmax_bits(g[l]), N, D)
        s_all.append(s)
        fin = np.isfinite(v)
        q = np.rint(np.ldexp(v[fin], np.int32(s))).astype(np.int64)
        np.add.at(acc, e[fin], q)
        bad[e[~fin]] = True
    for l in range(L):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        lo_e, hi_e = max(lo, 0) * F, min(max(hi, lo), n_rows) * F
        out[lo_e:hi_e] = np.ldexp(acc[lo_e:hi_e].astype(F32), np.int32(-s_all[l]))
        out[lo_e:hi_e][bad[lo_e:hi_e]] = np.nan
    gin = None
    if dy_dx is not None:
        dy = np.ascontiguousarray(dy_dx, F32).reshape(N, L, D, F)
        gin = np.zeros((N, D), F32)
        for l in range(L):
            for ch in range(F):
                gin = gin + g[l, :, ch][:, None] * dy[:, l, :, ch]
    return out.reshape(n_rows, F), gin, s_all


def fixed_point_bound(inputs, offsets, resolutions, n_rows, grad):
    """(float64 sum of the fp32 contributions, allowed |error| of the fixed-point result) per element: 0.5 ulp of the
    fp32 result + count 2^(-s - 1)."""
    g = np.ascontiguousarray(grad, F32)
    L, N, F = g.shape
    D = np.asarray(inputs).shape[1]
    s64 = np.zeros(n_rows * F, np.float64)
    cnt = np.zeros(n_rows * F, np.float64)
    slack = np.zeros(n_rows * F, np.float64)
    for l, (e, v) in enumerate(contributions(inputs, offsets, resolutions, n_rows, g)):
        s = scale_exp(level_gmax_bits(g[l]), N, D)
        np.add.at(s64, e, v.astype(np.float64))
        c = np.zeros(n_rows * F)
        np.add.at(c, e, 1.0)
        cnt += c
        slack += c * 2.0 ** (-s - 1)
    ulp_half = np.spacing(np.abs(s64).astype(F32)).astype(np.float64) * 0.5
    return s64.reshape(n_rows, F), (ulp_half + slack).reshape(n_rows, F), cnt.reshape(n_rows, F)


def forward_f64(inputs, embeddings, offsets, resolutions, fused_pos=False):
    """Independent float64 torch twin of the interpolation (output only) -> outputs [L, N, F] (torch, float64,
    differentiable in inputs if they require grad).  Plain dense / hashed indexing by python ints.  fused_pos: take the
    fp32 position rounded once (pos_fused: a contracting build) instead of the specification's two roundings."""
    import torch
    x = inputs
    N, D = x.shape
    emb = embeddings
    outs = []
    inside = ((x >= 0) & (x <= 1)).all(dim=1)
    for l in range(len(resolutions)):
        off, hs, res = int(offsets[l]), int(offsets[l + 1]) - int(offsets[l]), int(resolutions[l])
        pos = x * (res - 2) + 0.5
        # the position itself is an fp32 quantity of the spec (pos = x * float(res - 2) + 0.5 in fp32): take its value
        # from fp32, keep the float64 derivative
        if fused_pos:
            pos32 = torch.from_numpy(pos_fused(x.detach().float().numpy(), res)).double()
        else:
            pos32 = (x.detach().float() * float(res - 2) + 0.5).double()
        pos = pos + (pos32 - pos.detach())
        pg = torch.floor(pos).detach()
        fr = pos - pg
        pgi = pg.long()
        terms, wsum = [], torch.zeros(N, dtype=torch.float64)
        for k in range(1 << D):
            w = torch.ones(N, dtype=torch.float64)
            p = []
            for d in range(D):
                if (k >> d) & 1:
                    w = w * fr[:, d]
                    p.append(torch.clamp(pgi[:, d] + 1, max=res - 1))
                else:
                    w = w * (1 - fr[:, d])
                    p.append(pgi[:, d])
            ok = torch.ones(N, dtype=torch.bool)
            for d in range(D):
                ok &= (p[d] != 0) & (p[d] != res - 1)
            if res ** D <= hs:
                idx = sum(p[d] * res ** d for d in range(D))
            else:
                # the reference's rule: dense digits while the running stride fits, else the hash of all coordinates
                stride, dense = 1, True
                for d in range(D):
                    if stride > hs:
                        break
                    stride *= res
                dense = stride <= hs
                if dense:
                    idx = sum(p[d] * res ** d for d in range(D))
                else:
                    h = torch.zeros(N, dtype=torch.long)
                    for d in range(D):
                        h = h ^ ((p[d] * PRIMES[d]) & 0xFFFFFFFF)
                    idx = h
            idx = idx % hs
            wv = torch.where(ok, w, torch.zeros_like(w))
            wsum = wsum + wv
            terms.append((wv, emb[off + idx]))
        wsum = torch.where(wsum == 0, torch.full_like(wsum, 1e-9), wsum)
        o = sum(wv[:, None] / wsum[:, None] * e for wv, e in terms)
        o = torch.where(inside[:, None], o, torch.zeros_like(o))
        outs.append(o)
    return torch.stack(outs)
