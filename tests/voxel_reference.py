"""Plain numpy restatement of include/bloomscene_voxelize.h -- both quantisation rules, the validity rule, the key
packing, a stable sort and the emit -- and BloomScene's GM:824-862 (GaussianModel.anchor_growing,
scene/gaussian_model.py) written out in eager torch on whatever device its inputs live on."""
import numpy as np
import torch

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


class TooWide(ValueError):
    """The three spans need more than 64 key bits together."""


def quantise_ref(x, s, rule="divide"):
    """x float32 / float64 [n, 3] -> (q int32 [n, 3], valid bool [n]) in x's own type.  divide: rint(x / s), the division
    correctly rounded (numpy's is); reciprocal (float32 only): rint(x * float32(1.0 / s)), the reciprocal taken in double
    and rounded to float32 once (torch's GPU rule for tensor / python_scalar).
    np.rint rounds ties to even.  A row is invalid if a component is not finite or outside [-2^31, 2^31); its q is 0."""
    x = np.asarray(x)
    T = x.dtype.type
    assert x.dtype in (np.float32, np.float64)
    with np.errstate(all="ignore"):
        if rule == "divide":
            t = np.rint(x / T(s))
        else:
            assert rule == "reciprocal" and x.dtype == np.float32
            t = np.rint(x * np.float32(1.0 / float(s)))
        assert t.dtype == x.dtype
        inside = (t >= T(-2.0 ** 31)) & (t < T(2.0 ** 31))          # (False for NaN)
    valid = inside.all(axis=1)
    q = np.where(valid[:, None], np.where(inside, t, 0), 0).astype(np.int32)
    return q, valid


def key_layout(coords):
    """int32 [E, 3], E >= 1 -> (mins [3], bits [3]): each axis gets exactly the bits its span max - min needs."""
    c = np.asarray(coords, np.int64)
    mins = c.min(axis=0)
    bits = [int(int(span).bit_length()) for span in (c.max(axis=0) - mins)]
    return mins, bits


def pack_keys(coords):
    """-> (keys uint64 [E], mins, bits): (x - xmin) << (by + bz) | (y - ymin) << bz | (z - zmin).  Raises TooWide."""
    mins, bits = key_layout(coords)
    if sum(bits) > 64:
        raise TooWide(f"{bits[0]} + {bits[1]} + {bits[2]} = {sum(bits)} key bits")
    d = (np.asarray(coords, np.int64) - mins).astype(np.uint64)
    sx = bits[1] + bits[2]
    kx = d[:, 0] << np.uint64(sx) if sx < 64 else np.zeros(len(d), np.uint64)     # (then bx == 0: nothing to place)
    return kx | (d[:, 1] << np.uint64(bits[2])) | d[:, 2], mins, bits


def unpack_keys(keys, mins, bits):
    mask = lambda b: np.uint64((1 << b) - 1)
    sx = bits[1] + bits[2]
    x = keys >> np.uint64(sx) if sx < 64 else np.zeros(len(keys), np.uint64)
    y = (keys >> np.uint64(bits[2])) & mask(bits[1])
    z = keys & mask(bits[2])
    return (np.stack([x, y, z], 1).astype(np.int64) + mins).astype(np.int32)


def voxel_unique_ref(coords):
    """bsr_voxel_unique on int32 coordinates [E, 3] -> (coords [U, 3] int32, inverse [E], first [U], counts [U], int64):
    pack, a STABLE sort of (key, position), head flags, an inclusive scan, emit."""
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    E = coords.shape[0]
    if E == 0:
        z = np.zeros(0, np.int64)
        return np.zeros((0, 3), np.int32), z, z.copy(), z.copy()
    keys, mins, bits = pack_keys(coords)
    order = np.argsort(keys, kind="stable")                  # the payload: positions, ascending inside a key
    sk = keys[order]
    head = np.ones(E, bool)
    head[1:] = sk[1:] != sk[:-1]
    voxel = np.cumsum(head) - 1
    U = int(voxel[-1]) + 1
    inverse = np.empty(E, np.int64)
    inverse[order] = voxel
    start = np.flatnonzero(head)
    first = order[start].astype(np.int64)                    # stable: the smallest position of the voxel
    counts = np.diff(np.append(start, E)).astype(np.int64)
    assert len(first) == U
    return unpack_keys(sk[start], mins, bits), inverse, first, counts


def voxel_points_ref(coords, s, dtype):
    """T(c) * T(s), a zero always +0."""
    T = np.dtype(dtype).type
    p = coords.astype(dtype) * T(s)
    p[coords == 0] = 0
    return p


def unique_rows_ref(x, s, rows=None, rule="divide"):
    """The whole function on points: -> (n_invalid, result or None).  A rows entry outside [0, P) is invalid; a call
    with an invalid row produces the count and nothing else."""
    x = np.asarray(x)
    P = x.shape[0]
    rows = np.arange(P) if rows is None else np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < P)
    q, valid = quantise_ref(x[np.where(inside, rows, 0)], s, rule)
    valid &= inside
    if not valid.all():
        return int((~valid).sum()), None
    return 0, voxel_unique_ref(q)


def voxelize_sample_ref(data, s):
    """GaussianModel.voxelize_sample on the restatement: the voxel centres in the data's own type."""
    n_bad, res = unique_rows_ref(data, s)
    assert n_bad == 0
    return voxel_points_ref(res[0], s, np.asarray(data).dtype)


def voxelize_sample_numpy(data, s):
    """GM:437 written out (GM:436's shuffle does not change a unique)."""
    return np.unique(np.round(data / s), axis=0) * s


def grow_level_eager(anchor, offset, scaling, candidate_mask, anchor_feat, cur_size):
    """GM:824-862 of one level in eager torch, line for line, on the device of its inputs; torch's own scatter_reduce
    (amax) stands in for torch_scatter.scatter_max.  -> (candidate_anchor [M, 3], new_feat [M, F])."""
    N, K = offset.shape[0], offset.shape[1]
    feat_dim = anchor_feat.shape[1]
    all_xyz = anchor.unsqueeze(dim=1) + offset * scaling[:, :3].unsqueeze(dim=1)                  # GM:824
    grid_coords = torch.round(anchor / cur_size).int()                                            # GM:829
    selected_xyz = all_xyz.view([-1, 3])[candidate_mask]                                          # GM:831
    selected_grid_coords = torch.round(selected_xyz / cur_size).int()                             # GM:832
    unique_coords, inverse = torch.unique(selected_grid_coords, return_inverse=True, dim=0)       # GM:834
    occupied = torch.zeros(unique_coords.shape[0], dtype=torch.bool, device=anchor.device)
    for i in range(0, N, 4096):                                                                   # GM:838-847
        occupied |= (unique_coords.unsqueeze(1) == grid_coords[i:i + 4096]).all(-1).any(-1).view(-1)
    keep = ~occupied
    candidate_anchor = unique_coords[keep] * cur_size                                             # GM:850
    if candidate_anchor.shape[0] == 0:
        return candidate_anchor.float().reshape(0, 3), anchor_feat.new_zeros(0, feat_dim)
    new_feat = anchor_feat.unsqueeze(dim=1).repeat([1, K, 1]).view([-1, feat_dim])[candidate_mask]   # GM:861
    index = inverse.unsqueeze(1).expand(-1, feat_dim)
    out = anchor_feat.new_zeros(unique_coords.shape[0], feat_dim).scatter_reduce(0, index, new_feat, "amax",
                                                                                 include_self=False)   # GM:862
    return candidate_anchor, out[keep]


def boundary_points(n, sizes, seed, spread=2.0):
    """float32 [n, 3]: uniform points in a box of `spread` units, a third of whose components are moved to within 2 ulp
    of a rounding boundary (k + 0.5) * s of one of `sizes` -- the points tests/densify_reference.make_growth_case draws
    again -- and a few exactly representable ties and signed zeros."""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 3)) * spread - spread / 4).astype(np.float32)
    pick = rng.random((n, 3)) < 1 / 3
    s = np.asarray(sizes, np.float64)[rng.integers(0, len(sizes), (n, 3))]
    edge = ((np.floor(x / s) + 0.5) * s).astype(np.float32)
    ulps = rng.integers(-2, 3, (n, 3))
    moved = edge.copy()
    for k in (1, 2):
        up = np.nextafter(moved, np.float32(np.inf))
        dn = np.nextafter(moved, np.float32(-np.inf))
        moved = np.where(ulps >= k, up, np.where(ulps <= -k, dn, moved))
    x[pick] = moved[pick]
    x[:6, 0] = np.array([0.0, -0.0, 0.5, -0.5, 1.5, 2.5], np.float32)
    return x


def case_with_bits(bits, rng, E=400):
    """int32 rows whose spans need exactly bits[k] bits on axis k, at a random signed base."""
    cols = []
    for b in bits:
        span = (1 << b) - 1
        base = int(rng.integers(I32_MIN, I32_MAX - span + 1))
        v = rng.integers(0, span + 1, E).astype(np.int64) if span else np.zeros(E, np.int64)
        if span:
            v[:2] = [0, span]                            # both ends: the span is exactly this wide
        cols.append(v + base)
    c = np.stack(cols, 1)
    c[E // 2:] = c[rng.integers(0, E // 2, E - E // 2)]   # duplicates
    return c.astype(np.int32)
