"""Plain numpy / Python restatements of include/bloomscene_densify.h, and BloomScene's GM:829-862
(GaussianModel.anchor_growing, scene/gaussian_model.py) on CPU torch over them.

torch_scatter itself is not a dependency of this repository and its source is not vendored, so scatter_max_ref pins the
contract its documentation states -- empty groups give 0 and argmax == src.size(dim) -- plus the header's choices where
the extension is silent or racy: the first row wins a tie, NaN is above everything."""
import numpy as np
import torch

F32 = np.float32


def bits(a):
    """float32 array (numpy or torch) -> its uint32 bit patterns, for bit-for-bit comparisons."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, F32).view(np.uint32)


def scatter_max_ref(src, index, G, row_map=None):
    """bsr_scatter_max.  src [S, F] or [S] float32; index [E] or [E, F] integers; row_map [E] or None.
    -> (out float32, arg int64), [G, F] or [G].  One pass over the contributions in order: a contribution replaces the
    current winner only when it is STRICTLY above it (NaN above everything, NaN not above NaN, -0 == +0), so the first
    of the maximal rows stays."""
    src = np.ascontiguousarray(src, F32)
    one_d = src.ndim == 1
    src2 = src[:, None] if one_d else src
    S, F = src2.shape
    index = np.asarray(index, np.int64)
    E = index.shape[0]
    idx2 = np.broadcast_to(index[:, None] if index.ndim == 1 else index, (E, F))
    out_bits = np.zeros((G, F), np.uint32)   # (winners are copied as bit patterns: the sign of a zero, a NaN's payload)
    out = out_bits.view(F32)
    arg = np.full((G, F), E, np.int64)
    src_bits = src2.view(np.uint32)
    cols = np.arange(F)
    for e in range(E):
        r = e if row_map is None else int(row_map[e])
        if r < 0 or r >= S:
            continue
        v = src2[r]
        g = idx2[e]
        ok = (g >= 0) & (g < G)
        gc = np.where(ok, g, 0)
        cur, has = out[gc, cols], arg[gc, cols] != E
        with np.errstate(invalid="ignore"):
            above = (np.isnan(v) & ~np.isnan(cur)) | (v > cur)
        take = ok & (~has | above)
        out_bits[gc[take], cols[take]] = src_bits[r][take]
        arg[gc[take], cols[take]] = e
    if one_d:
        return out[:, 0], arg[:, 0]
    return out, arg


def order_key(b):
    """scatter_order_key of csrc/densify.hip on uint32 bit patterns: the 32-bit key whose unsigned order is the header's
    order of values (NaN above everything and all NaNs equal, -0 == +0)."""
    b = np.asarray(b, np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xffffffff), key).astype(np.uint32)


def scatter_max_packed(src, index, G, row_map=None):
    """The kernels' route to the same function: the maximum of key << 32 | (0xffffffff - e) per (g, f), unpacked.
    1-D index only."""
    src = np.ascontiguousarray(src, F32)
    S, F = src.shape
    E = len(index)
    packed = np.zeros((G, F), np.uint64)
    for e in range(E):
        g = int(index[e])
        r = e if row_map is None else int(row_map[e])
        if not (0 <= g < G and 0 <= r < S):
            continue
        v = (order_key(src[r].view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.uint64(0xffffffff - e)
        packed[g] = np.maximum(packed[g], v)
    arg = np.where(packed == 0, E, 0xffffffff - (packed & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int64)
    rows = arg if row_map is None else np.asarray(row_map, np.int64)[np.minimum(arg, max(E - 1, 0))]
    out_bits = np.where(packed == 0, 0, src.view(np.uint32)[np.where(packed == 0, 0, rows), np.arange(F)[None, :]])
    return out_bits.astype(np.uint32).view(F32), arg


def voxel_isin_ref(query, keys):
    """bsr_voxel_isin: membership of each query row in the SET of key rows."""
    have = {tuple(int(c) for c in row) for row in np.asarray(keys).reshape(-1, 3)}
    return np.array([tuple(int(c) for c in row) in have for row in np.asarray(query).reshape(-1, 3)], bool)


def grow_candidates_ref(anchor, all_xyz, candidate_mask, anchor_feat, cur_size, n_offsets):
    """GM:829-862 on CPU tensors, line for line (the chunked all-pairs comparison, the repeated feature tensor), with
    scatter_max_ref standing in for torch_scatter.  -> (candidate_anchor [M, 3], new_feat [M, F]); two empty tensors
    where GM:852 skips the level."""
    feat_dim = anchor_feat.shape[1]
    grid_coords = torch.round(anchor / cur_size).int()
    selected_xyz = all_xyz.view([-1, 3])[candidate_mask]
    selected_grid_coords = torch.round(selected_xyz / cur_size).int()
    selected_grid_coords_unique, inverse_indices = torch.unique(selected_grid_coords, return_inverse=True, dim=0)
    chunk_size = 4096
    max_iters = grid_coords.shape[0] // chunk_size + (1 if grid_coords.shape[0] % chunk_size != 0 else 0)
    remove_duplicates = torch.zeros(selected_grid_coords_unique.shape[0], dtype=torch.bool)
    for i in range(max_iters):
        cur = (selected_grid_coords_unique.unsqueeze(1) == grid_coords[i * chunk_size:(i + 1) * chunk_size, :]) \
            .all(-1).any(-1).view(-1)
        remove_duplicates = torch.logical_or(remove_duplicates, cur)
    remove_duplicates = ~remove_duplicates
    candidate_anchor = selected_grid_coords_unique[remove_duplicates] * cur_size
    if candidate_anchor.shape[0] == 0:
        return torch.empty(0, 3), torch.empty(0, feat_dim)
    new_feat = anchor_feat.unsqueeze(dim=1).repeat([1, n_offsets, 1]).view([-1, feat_dim])[candidate_mask]
    index = inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1))
    out, _ = scatter_max_ref(new_feat.numpy(), index.numpy(), selected_grid_coords_unique.shape[0])
    return candidate_anchor, torch.from_numpy(out)[remove_duplicates]


def _near_half(x, cur_sizes, margin=1e-4):
    bad = torch.zeros(x.shape, dtype=torch.bool)
    for s in cur_sizes:
        q = x.double() / s
        bad |= (q - torch.floor(q) - 0.5).abs() < margin
    return bad


def make_growth_case(N, K, F, seed, cur_sizes, fraction=0.05):
    """A seeded anchor_growing level on CPU tensors: anchors uniform in a 2-unit box, K offsets around each, a `fraction`
    candidate mask, normal features.  torch divides by a Python scalar as x * (1 / s) on the GPU and as x / s on the CPU,
    up to 2 ulp of a quotient below 256 apart (3e-5), so coordinates whose quotient by one of `cur_sizes` lies within
    1e-4 of a rounding boundary of torch.round are drawn again: the voxel of every point is the same on both."""
    g = torch.Generator().manual_seed(seed)
    anchor = torch.rand(N, 3, generator=g) * 2.0
    while True:
        bad = _near_half(anchor, cur_sizes)
        if not bad.any():
            break
        anchor[bad] = torch.rand(int(bad.sum()), generator=g) * 2.0
    offsets = (torch.rand(N, K, 3, generator=g) - 0.5) * 0.3
    while True:
        all_xyz = anchor.unsqueeze(1) + offsets
        bad = _near_half(all_xyz, cur_sizes)
        if not bad.any():
            break
        offsets[bad] = (torch.rand(int(bad.sum()), generator=g) - 0.5) * 0.3
    mask = torch.rand(N * K, generator=g) < fraction
    feat = torch.randn(N, F, generator=g)
    return anchor, all_xyz, mask, feat
