"""CPU restatement of include/bloomscene_knn.h (BloomScene's ``simple_knn._C.distCUDA2``): the mean of the three smallest
squared distances from every point to the others.

    d(i, j) = (dx*dx + dy*dy) + dz*dz,  dx = p_j.x - p_i.x etc.   fp32, every operation rounded
    C(i)    = { d(i, j) : j != i, d(i, j) < FLT_MAX }
    out[i]  = ((s0 + s1) + s2) / 3   (s0 <= s1 <= s2 the three smallest of C(i), padded with FLT_MAX; division
                                      correctly rounded)

``mean_dist3_numpy`` is a brute force in numpy fp32 (every ufunc call rounds once).  ``mean_dist3_torch`` is the same
brute force built from separate elementwise torch ops, which no backend contracts, so it is bit-exact on any device;
the division goes through float64 (53 >= 2 * 24 + 2 bits: rounding twice equals rounding once).  ``mean_dist3_f64`` is
the float64 twin.  ``box_bound_point`` / ``box_bound_range`` restate the kernels' pruning bounds (csrc/knn.hip).
"""
import numpy as np
import torch

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)


def _finish_numpy(d):
    """d [n, m] fp32 candidate values (invalid ones already FLT_MAX) -> fp32 [n]."""
    if d.shape[1] < 3:
        d = np.concatenate([d, np.full((d.shape[0], 3 - d.shape[1]), FLT_MAX, F32)], axis=1)
    s = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) / F32(3.0)


def mean_dist3_numpy(points, chunk=512):
    p = np.ascontiguousarray(points, F32)
    P = p.shape[0]
    out = np.empty(P, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, P, chunk):
            b = min(P, a + chunk)
            q = p[a:b]
            dx = p[None, :, 0] - q[:, None, 0]
            dy = p[None, :, 1] - q[:, None, 1]
            dz = p[None, :, 2] - q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d = np.where(d < FLT_MAX, d, FLT_MAX)
            d[np.arange(b - a), np.arange(a, b)] = FLT_MAX   # j != i
            out[a:b] = _finish_numpy(d.astype(F32))
    return out


def mean_dist3_torch(points, chunk=256, return_sums=False):
    """points float32 [P, 3] on any device -> float32 [P] on that device (bit-equal to mean_dist3_numpy)."""
    p = points.contiguous().float()
    P = p.shape[0]
    dev = p.device
    fmax = torch.tensor(float(FLT_MAX), dtype=torch.float32, device=dev)
    sums = torch.empty(P, dtype=torch.float32, device=dev)
    px, py, pz = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    for a in range(0, P, chunk):
        b = min(P, a + chunk)
        dx = torch.sub(px[None, :], px[a:b, None])
        d = torch.mul(dx, dx)
        del dx
        dy = torch.sub(py[None, :], py[a:b, None])
        d = torch.add(d, torch.mul(dy, dy))
        del dy
        dz = torch.sub(pz[None, :], pz[a:b, None])
        d = torch.add(d, torch.mul(dz, dz))
        del dz
        d = torch.where(d < fmax, d, fmax)
        r = torch.arange(b - a, device=dev)
        d[r, r + a] = fmax
        if P < 3:
            d = torch.cat([d, fmax.expand(b - a, 3 - P)], dim=1)
        s = torch.topk(d, 3, dim=1, largest=False, sorted=True).values
        sums[a:b] = torch.add(torch.add(s[:, 0], s[:, 1]), s[:, 2])
    if return_sums:
        return sums
    return (sums.double() / 3.0).float()


def mean_dist3_f64(points):
    """Float64 twin: the same selection rule with distances in float64 (no rounding of d), result in float64."""
    p = np.asarray(points, np.float64)
    P = p.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        d = ((p[None, :, :] - p[:, None, :]) ** 2).sum(-1)
    fmax = float(FLT_MAX)
    d = np.where(d < fmax, d, fmax)
    d[np.arange(P), np.arange(P)] = fmax
    if P < 3:
        d = np.concatenate([d, np.full((P, 3 - P), fmax)], axis=1)
    s = np.sort(d, axis=1)[:, :3]
    return s.sum(1) / 3.0


def _gap_point(p, lo, hi):
    return np.where(p < lo, lo - p, np.where(p > hi, p - hi, F32(0)))


def box_bound_point(p, lo, hi):
    """The kernels' per-lane bound of d(p, q) over q in [lo, hi] (fp32, the operation order of d)."""
    p, lo, hi = (np.asarray(v, F32) for v in (p, lo, hi))
    with np.errstate(over="ignore"):
        g = [_gap_point(p[..., k], lo[..., k], hi[..., k]) for k in range(3)]
        return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def box_bound_range(qlo, qhi, lo, hi):
    """The kernels' wave-level bound of d(p, q) over p in [qlo, qhi] and q in [lo, hi]."""
    qlo, qhi, lo, hi = (np.asarray(v, F32) for v in (qlo, qhi, lo, hi))
    with np.errstate(over="ignore"):
        g = [np.where(qhi[..., k] < lo[..., k], lo[..., k] - qhi[..., k],
                      np.where(qlo[..., k] > hi[..., k], qlo[..., k] - hi[..., k], F32(0))) for k in range(3)]
        return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def pair_dist(p, q):
    """d(p, q) of the spec, fp32, elementwise over [..., 3] arrays (dx = q - p)."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (q[..., k] - p[..., k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


# ---- inputs shared by the CPU and GPU tests ----

def make_cloud(kind, P, seed=0):
    """float32 [P, 3] test inputs: uniform, planar, collinear, identical, duplicates, clusters, offset, nonfinite,
    surface (a few noisy depth surfaces, planar pieces, ~5 % exact duplicates)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x = rng.uniform(-1, 1, (P, 3))
    elif kind == "planar":
        x = rng.uniform(-1, 1, (P, 3))
        x[:, 2] = 0.25
    elif kind == "collinear":
        t = rng.uniform(-1, 1, (P, 1))
        x = np.array([0.3, -0.2, 0.7]) + t * np.array([1.0, 2.0, -0.5])
    elif kind == "identical":
        x = np.tile(np.array([[0.1, -2.0, 3.5]]), (P, 1))
    elif kind == "duplicates":
        base = rng.uniform(-1, 1, (max(1, P // 8), 3))
        x = base[rng.integers(0, base.shape[0], P)]
    elif kind == "clusters":
        centres = rng.uniform(-1000, 1000, (5, 3))
        x = centres[rng.integers(0, 5, P)] + rng.normal(0, 1e-3, (P, 3))
    elif kind == "offset":
        x = rng.uniform(-1, 1, (P, 3)) + rng.choice([-1e6, 1e6], (P, 3))
    elif kind == "nonfinite":
        x = rng.uniform(-1, 1, (P, 3))
        if P >= 2:
            n = max(1, P // 16)
            idx = rng.choice(P, n, replace=False)
            vals = np.array([np.nan, np.inf, -np.inf])
            x[idx, rng.integers(0, 3, n)] = vals[rng.integers(0, 3, n)]
    elif kind == "surface":
        x = surface_cloud(P, rng)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, F32)


def surface_cloud(P, rng):
    """BloomScene-like: unprojected depth surfaces (a few noisy height fields), planar pieces, ~5 % exact duplicates."""
    n_dup = P // 20
    n = P - n_dup
    parts = []
    k = 4
    for s in range(k):
        m = n // (k + 2) if s < k - 1 else n - (k - 1) * (n // (k + 2)) - 2 * (n // (k + 2))
        u, v = rng.uniform(-1, 1, (2, m))
        h = 0.3 * np.sin(3 * u + s) * np.cos(2 * v - s) + rng.normal(0, 2e-3, m)
        parts.append(np.stack([u + 0.5 * s, v, h + s], 1))
    for s in range(2):
        m = n // (k + 2)
        u, v = rng.uniform(-1, 1, (2, m))
        parts.append(np.stack([u, np.full(m, 2.0 + s), v], 1))   # planar: zero extent in y
    x = np.concatenate(parts, 0)
    x = np.round(x / 1e-3) * 1e-3                                # voxelised at 0.001
    if n_dup:
        x = np.concatenate([x, x[rng.integers(0, x.shape[0], n_dup)]], 0)
    return x[rng.permutation(x.shape[0])]
