"""The device steps of BloomScene's anchor densification on the MI355X (``GaussianModel.anchor_growing``,
``scene/gaussian_model.py:807-895``, "GM"), in HIP behind ``include/bloomscene_densify.h``.

    out, argmax = scatter_max(src, index, dim_size, row_map=None)   # torch_scatter.scatter_max along dim 0 (GM:862)
    occupied    = voxel_isin(query, keys)                           # GM:838-849 before its negation
    candidate_anchor, new_feat = grow_candidates(anchor, all_xyz, candidate_mask, anchor_feat, cur_size)   # GM:829-862

``scatter_max`` is a pure function of its input, written out in the header: the first row wins a tie, NaN is above
everything, an empty group gives ``0`` and ``argmax == E`` (torch_scatter's convention), index entries out of range
contribute nothing.  It is bit-identical from run to run.  All three run on the current torch stream;
``scatter_max`` and ``voxel_isin`` make no host synchronisation (capturable into a CUDA graph) and take their scratch
from torch's allocator.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _capi
from . import _operands as _ops
from .grid_encoder import check_call


def scatter_max(src: torch.Tensor, index: torch.Tensor, dim_size: int, row_map: torch.Tensor | None = None):
    """Column-wise maximum per group along dimension 0 and the contribution it came from (``bsr_scatter_max``).

    ``src`` float32 ``[S, F]`` or ``[S]``; ``index`` int64 ``[E]`` or ``[E, F]`` with any non-negative strides (a
    stride-0 ``.expand(-1, F)`` view is read in place); ``row_map`` int64 ``[E]`` or None (then ``S == E``):
    contribution ``e`` reads ``src[row_map[e]]``.  -> ``out`` float32 and ``argmax`` int64, ``[dim_size, F]`` (or
    ``[dim_size]`` for a 1-D ``src``); ``argmax`` numbers contributions, not source rows."""
    who = "scatter_max"
    _ops.check_tensors(who, [("src", src)], None)
    if src.dim() not in (1, 2):
        raise ValueError(f"{who}: src must be [S] or [S, F] (got {list(src.shape)})")
    one_d = src.dim() == 1
    src = src.detach().contiguous()
    _ops.check_tensors(who, [("src", src)], half_note=False)
    ints = [("index", index)] + ([] if row_map is None else [("row_map", row_map)])
    _ops.check_tensors(who, ints, torch.int64)       # (every dtype before any device, as in _operands)
    _ops.check_on_gpu(who, ints)
    check_call(who, 3, 1, float_tensors=(("src", src),))   # off the GPU ValueError
    S, F = src.shape[0], (1 if one_d else src.shape[1])
    G = int(dim_size)
    if G < 0:
        raise ValueError(f"{who}: dim_size must be >= 0 (got {dim_size})")
    if F < 1:
        raise ValueError(f"{who}: src must have at least one column (got {list(src.shape)})")
    if index.dim() == 1:
        E, is0, is1 = index.shape[0], index.stride(0), 0
    elif index.dim() == 2 and not one_d and index.shape[1] == F:
        E, is0, is1 = index.shape[0], index.stride(0), index.stride(1)
    else:
        raise ValueError(f"{who}: index must be [E] or [E, {F}] for src {list(src.shape)} (got {list(index.shape)})")
    if row_map is None:
        if E != S:
            raise ValueError(f"{who}: index has {E} rows, src {S} (pass row_map to read rows more than once)")
    else:
        if row_map.dim() != 1 or row_map.shape[0] != E:
            raise ValueError(f"{who}: row_map must be [{E}] (got {list(row_map.shape)})")
        row_map = row_map.contiguous()
    if E >= 2 ** 31 or S >= 2 ** 31 or G * F >= 2 ** 31:
        raise ValueError(f"{who}: need E, S and dim_size * F below 2^31 (got {E}, {S}, {G} * {F})")
    shape = (G,) if one_d else (G, F)
    if G == 0 or E == 0:   # nothing to reduce: the empty result
        return (torch.zeros(shape, dtype=torch.float32, device=src.device),
                torch.full(shape, E, dtype=torch.int64, device=src.device))
    out = torch.empty(shape, dtype=torch.float32, device=src.device)
    arg = torch.empty(shape, dtype=torch.int64, device=src.device)
    _capi.call("bsr_scatter_max", E, S, F, G, src.data_ptr(), _ops.ptr(row_map), index.data_ptr(), is0, is1,
               out.data_ptr(), arg.data_ptr(), _ops.stream(src.device))
    return out, arg


def voxel_isin(query: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """``query`` int32 ``[U, 3]``, ``keys`` int32 ``[N, 3]`` on the GPU -> bool ``[U]``: row ``u`` of ``query`` equals some
    row of ``keys`` in all three components (``bsr_voxel_isin``).  ``keys`` may repeat rows."""
    who = "voxel_isin"
    for name, t in (("query", query), ("keys", keys)):
        _ops.check_tensors(who, [(name, t)], None)
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be [n, 3] (got {list(t.shape)})")
    query, keys = query.contiguous(), keys.contiguous()
    check_call(who, 3, 1, int_tensors=(("query", query), ("keys", keys)))   # dtype TypeError, off the GPU ValueError
    U, N = query.shape[0], keys.shape[0]
    if U == 0 or N == 0:
        return torch.zeros(U, dtype=torch.bool, device=query.device)
    nbytes = _capi.lib().bsr_voxel_isin_scratch_bytes(N)
    if nbytes == 0:
        raise ValueError(f"{who}: too many keys ({N})")
    mask = torch.empty(U, dtype=torch.uint8, device=query.device)
    scratch = _ops.scratch(nbytes, query.device)
    _capi.call("bsr_voxel_isin", U, N, query.data_ptr(), keys.data_ptr(), mask.data_ptr(), scratch.data_ptr(),
               _ops.stream(query.device))
    return mask.view(torch.bool)


@torch.no_grad()
def grow_candidates(anchor: torch.Tensor, all_xyz: torch.Tensor, candidate_mask: torch.Tensor,
                    anchor_feat: torch.Tensor, cur_size: float):
    """GM:829-862 of one ``anchor_growing`` level, without the all-pairs comparison of GM:838-847 and without the
    ``[N * K, F]`` tensor of GM:861.

    ``anchor`` float32 ``[N, 3]``; ``all_xyz`` float32 ``[N, K, 3]`` or ``[N * K, 3]`` (GM:824); ``candidate_mask`` bool
    ``[N * K]``; ``anchor_feat`` float32 ``[N, F]``; ``cur_size`` the level's voxel size (GM:827).  -> ``candidate_anchor``
    float32 ``[M, 3]`` (GM:850) and ``new_feat`` float32 ``[M, F]`` (GM:861-862, bit-equal), rows in ``torch.unique``'s
    order.  No candidates: two empty tensors (GM:852 then skips the level)."""
    who = "grow_candidates"
    if anchor.dim() != 2 or anchor.shape[1] != 3:
        raise ValueError(f"{who}: anchor must be [N, 3] (got {list(anchor.shape)})")
    N = anchor.shape[0]
    flat_xyz = all_xyz.reshape(-1, 3)
    if anchor_feat.dim() != 2 or anchor_feat.shape[0] != N:
        raise ValueError(f"{who}: anchor_feat must be [{N}, F] (got {list(anchor_feat.shape)})")
    if N == 0 or flat_xyz.shape[0] % N != 0:
        raise ValueError(f"{who}: all_xyz must hold K offsets for each of the {N} anchors (got {list(all_xyz.shape)})")
    K = flat_xyz.shape[0] // N
    if candidate_mask.dtype != torch.bool or tuple(candidate_mask.shape) != (N * K,):
        raise ValueError(f"{who}: candidate_mask must be bool [{N * K}] (got {candidate_mask.dtype} "
                         f"{list(candidate_mask.shape)})")
    F = anchor_feat.shape[1]
    grid_coords = torch.round(anchor / cur_size).int()                                   # GM:829
    selected = candidate_mask.nonzero().squeeze(1)                                        # flat offset numbers
    selected_grid_coords = torch.round(flat_xyz[selected] / cur_size).int()              # GM:831-832
    unique_coords, inverse = torch.unique(selected_grid_coords, return_inverse=True, dim=0)   # GM:834
    keep = ~voxel_isin(unique_coords, grid_coords)                                        # GM:838-849
    candidate_anchor = unique_coords[keep] * cur_size                                     # GM:850
    if candidate_anchor.shape[0] == 0:
        return (torch.empty(0, 3, dtype=torch.float32, device=anchor.device),
                torch.empty(0, F, dtype=torch.float32, device=anchor.device))
    # GM:861-862: offset j of the flat list belongs to anchor j // K
    out, _ = scatter_max(anchor_feat, inverse, unique_coords.shape[0], row_map=selected // K)
    return candidate_anchor, out[keep]
