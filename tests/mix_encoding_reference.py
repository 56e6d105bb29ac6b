"""CPU restatement of the fused mixed 3D/2D binary hash-grid encoding of include/bloomscene_mix_grid.h (test
infrastructure), built on tests/grid_reference.py: numpy, fp32, every operation in the header's order.  The GPU forward,
dy_dx, table gradients and grad_x are bit-equal to `forward` / `backward`.
"""
from __future__ import annotations

import numpy as np

import grid_reference as GR

F32 = np.float32
MIX_DIMS = ((0, 1, 2), (0, 1), (0, 2), (1, 2))


def normalise(x, bound_min=None, bound_max=None):
    """u = (x - min) / (max - min): two fp32 subtractions and a correctly rounded division (numpy's); x without bounds."""
    x = np.ascontiguousarray(x, F32)
    if bound_min is None:
        return x
    lo, hi = np.asarray(bound_min, F32).reshape(1, 3), np.asarray(bound_max, F32).reshape(1, 3)
    return ((x - lo) / (hi - lo)).astype(F32)


def sign_table(params):
    """The value a corner reads with `binary`: +1 for p >= 0 (-0 included), -1 for p < 0, 0 for NaN."""
    p = np.asarray(params, F32)
    with np.errstate(invalid="ignore"):
        return np.where(p >= 0, F32(1), np.where(p < 0, F32(-1), F32(0))).astype(F32)


def gate(params):
    """STE_binary's backward mask: |p| <= 1, false for NaN."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(params, F32)) <= F32(1)


def _layout(tables, dims):
    """Per grid (first out column, first dy_dx column, L, D); C; W."""
    F = tables[0][0].shape[1]
    c = w = 0
    spans = []
    for (p, o, r), d in zip(tables, dims):
        L, D = len(r), len(d)
        spans.append((c, w, L, D))
        c += L * F
        w += L * D * F
    return spans, c, w, F


def forward(x, tables, dims, bound_min=None, bound_max=None, binary=True):
    """tables: [(params [R, F], offsets [L + 1], resolutions [L]), ...] -> out [n, C], dy_dx [n, W]."""
    u = normalise(x, bound_min, bound_max)
    n = u.shape[0]
    spans, C, W, F = _layout(tables, dims)
    out, dy = np.zeros((n, C), F32), np.zeros((n, W), F32)
    if n == 0:
        return out, dy
    for (p, o, r), d, (c0, w0, L, D) in zip(tables, dims, spans):
        emb = sign_table(p) if binary else np.asarray(p, F32)
        o_g, dy_g = GR.forward(np.ascontiguousarray(u[:, list(d)]), emb, o, r)
        out[:, c0:c0 + L * F] = o_g.transpose(1, 0, 2).reshape(n, L * F)
        dy[:, w0:w0 + L * D * F] = dy_g.reshape(n, L * D * F)
    return out, dy


def backward(x, tables, dims, grad_out, dy_dx=None, bound_min=None, bound_max=None, binary=True, gated=True, terms=None):
    """-> [grad_params_g [R_g, F]], grad_x [n, 3] (None without dy_dx).  gated=False: the table gradients before the gate.
    terms: a list that receives, per grid, r_g [n, 3] (0 in the coordinates the grid does not select)."""
    u = normalise(x, bound_min, bound_max)
    n = u.shape[0]
    spans, C, W, F = _layout(tables, dims)
    g_out = np.ascontiguousarray(grad_out, F32)
    grads, grad_u, seen = [], np.zeros((n, 3), F32), [False] * 3
    for (p, o, r), d, (c0, w0, L, D) in zip(tables, dims, spans):
        R = np.asarray(p).shape[0]
        if n == 0:
            grads.append(np.zeros((R, F), F32))
            continue
        g = np.ascontiguousarray(g_out[:, c0:c0 + L * F].reshape(n, L, F).transpose(1, 0, 2))
        dy_g = None if dy_dx is None else np.ascontiguousarray(dy_dx[:, w0:w0 + L * D * F]).reshape(n, L, D, F)
        ge, gi, _ = GR.backward(np.ascontiguousarray(u[:, list(d)]), o, r, R, g, dy_g)
        if binary and gated:
            ge = np.where(gate(p), ge, F32(0)).astype(F32)
        grads.append(ge)
        if gi is not None:
            if terms is not None:
                r = np.zeros((n, 3), F32)
                r[:, list(d)] = gi
                terms.append(r)
            for k, dd in enumerate(d):
                grad_u[:, dd] = grad_u[:, dd] + gi[:, k] if seen[dd] else gi[:, k]
                seen[dd] = True
    if dy_dx is None:
        return grads, None
    if bound_min is not None:
        lo, hi = np.asarray(bound_min, F32).reshape(1, 3), np.asarray(bound_max, F32).reshape(1, 3)
        with np.errstate(invalid="ignore", divide="ignore"):
            grad_u = (grad_u / (hi - lo)).astype(F32)
    return grads, grad_u
