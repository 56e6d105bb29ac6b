"""Which anchors exist: "quantise points to a voxel lattice and keep each voxel once" on the MI355X, in HIP behind
``include/bloomscene_voxelize.h`` (``GaussianModel.voxelize_sample``, ``scene/gaussian_model.py:435-438``, and GM:824-862
of ``anchor_growing``; "GM").

    coords, inverse, first, counts = voxel_unique(points_or_coords, voxel_size, rows=None, rule="divide")
    q                              = quantise(points, voxel_size, rule="divide")       # torch.round(x / s).int()
    anchors                        = voxelize_sample(data, voxel_size)                  # GM:435-438, numpy or tensor
    candidate_anchor, new_feat     = grow_level(anchor, offset, scaling, candidate_mask, anchor_feat, cur_size)

The function is written out per row in the header: two quantisation rules (``"divide"``: ``rint(x / s)``, numpy's and
torch's CPU rule; ``"reciprocal"``: ``rintf(x * float(1.0 / s))``, the reciprocal taken in double and rounded once,
what torch's GPU kernel computes for ``tensor / python_scalar``), voxels in ``np.unique(axis=0)`` /
``torch.unique(dim=0)`` order, ``first`` the smallest position of a voxel, everything bit-identical from run to run.  A row that does not quantise to an int32 (NaN, infinity,
``|q| >= 2^31``, a ``rows`` entry outside the source) and a coordinate range that needs more than 64 key bits raise
``ValueError``.  Everything runs on the current torch stream with memory from torch's allocator; ``voxel_unique`` ends in
ONE host read (``U`` and the status), ``quantise`` in none (capturable into a CUDA graph).  There is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from . import _operands as _ops

# include/bloomscene_voxelize.h
FORM_COORDS, FORM_POINTS_F, FORM_POINTS_D, FORM_COMPOSITE = 0, 1, 2, 3
RULES = {"divide": 0, "reciprocal": 1}
REFUSED_INVALID, REFUSED_WIDE = 1, 2
FLAG_TEST_SMALL_CHUNK = 0x100


def _check_source(who, x, rows, rule, want_coords, before_device=None):
    """The checks before any native call, in ``_operands``' order of complaints (``before_device`` makes the caller's
    shape and value checks).  -> the form."""
    _ops.check_tensors(who, [("the input", x)], None)
    allowed = (torch.float32, torch.float64, torch.int32) if want_coords else (torch.float32, torch.float64)
    if x.dtype not in allowed:
        raise TypeError(f"{who}: the input must be float32, float64{' or int32' if want_coords else ''} (got {x.dtype})")
    if rows is not None:
        _ops.check_tensors(who, [("rows", rows)], torch.int64)
    if rule not in RULES:
        raise ValueError(f"{who}: rule must be 'divide' or 'reciprocal' (got {rule!r})")
    if rule == "reciprocal" and x.dtype == torch.float64:
        raise NotImplementedError(f"{who}: rule='reciprocal' is float32 only (torch's GPU kernel divides float64 tensors "
                                  "by a scalar the same way, but no caller does)")
    if rows is not None and x.dtype == torch.int32:
        raise NotImplementedError(f"{who}: rows is not supported for int32 coordinates")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: the input must be [n, 3] (got {list(x.shape)})")
    if rows is not None and rows.dim() != 1:
        raise ValueError(f"{who}: rows must be [E] (got {list(rows.shape)})")
    if x.shape[0] >= 2 ** 31 or (rows is not None and rows.shape[0] >= 2 ** 31):
        raise ValueError(f"{who}: need fewer than 2^31 rows")
    if before_device is not None:
        before_device()
    _ops.check_on_gpu(who, [("the input", x)] + ([("rows", rows)] if rows is not None else []))
    return {torch.int32: FORM_COORDS, torch.float32: FORM_POINTS_F, torch.float64: FORM_POINTS_D}[x.dtype]


def _check_size(who, voxel_size):
    s = float(voxel_size)
    if not (s == s and s != 0.0 and abs(s) != float("inf")):
        raise ValueError(f"{who}: voxel_size must be finite and not 0 (got {voxel_size})")
    return s


def _strided_rows(x):
    """A [P, 3] tensor the kernels can read in place (unit column stride, a row stride of at least 3), else a copy."""
    if x.shape[0] > 0 and (x.stride(1) != 1 or x.stride(0) < 3):
        x = x.contiguous()
    return x, _ops.row_stride(x, x.shape[0], 3)


class _Source:
    """The source arguments of both entry points (form, P, src, stride, anchor, scaling, stride, K, rows)."""

    def __init__(self, form, P, src, stride=3, anchor=None, scaling=None, scaling_stride=0, K=0, rows=None):
        self.form, self.P, self.src, self.stride = form, P, src, stride
        self.anchor, self.scaling, self.scaling_stride, self.K, self.rows = anchor, scaling, scaling_stride, K, rows
        self.E = P if rows is None else rows.shape[0]
        self.device = src.device
        self.point_dtype = torch.float64 if form == FORM_POINTS_D else torch.float32

    def args(self, rule, voxel_size):
        ptr = _ops.ptr
        return (self.form, RULES[rule], self.E, self.P, ptr(self.src), self.stride, ptr(self.anchor), ptr(self.scaling),
                self.scaling_stride, self.K, ptr(self.rows), float(voxel_size))


def _point_source(who, x, rows, rule, want_coords, voxel_size, size_optional=False):
    def check_size():
        if voxel_size is None and not (size_optional and x.dtype == torch.int32):
            raise ValueError(f"{who}: voxel_size is required for points and for return_points")
        if voxel_size is not None:
            _check_size(who, voxel_size)
    form = _check_source(who, x, rows, rule, want_coords, check_size)
    x = x.detach()
    if form == FORM_COORDS:
        return _Source(form, x.shape[0], x.contiguous())
    x, stride = _strided_rows(x)
    return _Source(form, x.shape[0], x, stride, rows=None if rows is None else rows.contiguous())


def _quantise(src, voxel_size, rule):
    q = torch.empty(src.E, 3, dtype=torch.int32, device=src.device)
    if src.E:
        _capi.call("bsr_voxel_quantise", *src.args(rule, voxel_size), q.data_ptr(), None, _ops.stream(src.device))
    return q


def _unique(who, src, voxel_size, rule, return_points, flags=0):
    """bsr_voxel_unique on a checked source -> (coords, inverse, first, counts[, points]), the first U rows as views."""
    E, dev = src.E, src.device
    coords = torch.empty(E, 3, dtype=torch.int32, device=dev)
    inverse = torch.empty(E, dtype=torch.int64, device=dev)
    first = torch.empty(E, dtype=torch.int64, device=dev)
    counts = torch.empty(E, dtype=torch.int64, device=dev)
    points = torch.empty(E, 3, dtype=src.point_dtype, device=dev) if return_points else None
    U = 0
    if E:
        nbytes = _capi.lib().bsr_voxel_unique_scratch_bytes(E)
        if nbytes == 0:
            raise ValueError(f"{who}: too many rows ({E})")
        status = torch.empty(8, dtype=torch.int32, device=dev)
        scratch = _ops.scratch(nbytes, dev)
        _capi.call("bsr_voxel_unique", *src.args(rule, voxel_size if voxel_size is not None else 1.0),
                   coords.data_ptr(), inverse.data_ptr(), first.data_ptr(), counts.data_ptr(), _ops.ptr(points),
                   status.data_ptr(), scratch.data_ptr(), flags, _ops.stream(dev))
        st = [v & 0xffffffff for v in status.tolist()]          # the call's one host read
        raise_status(who, st)
        U = st[0]
    out = (coords[:U], inverse, first[:U], counts[:U])
    return out + (points[:U],) if return_points else out


def raise_status(who, st):
    """The status words of bsr_voxel_unique -> ValueError for a refused call."""
    if st[3] & REFUSED_INVALID:
        raise ValueError(f"{who}: {st[1]} invalid row(s): a coordinate that is not finite or outside [-2^31, 2^31) after "
                         "quantisation, or a rows entry outside the source")
    if st[3] & REFUSED_WIDE:
        raise ValueError(f"{who}: the coordinate ranges need {st[4]} + {st[5]} + {st[6]} = {st[2]} key bits, more than 64")


@torch.no_grad()
def voxel_unique(points_or_coords, voxel_size=None, rows=None, rule="divide", return_points=False, _flags=0):
    """The distinct voxels of the rows (``bsr_voxel_unique``).

    ``points_or_coords`` int32 ``[E, 3]`` coordinates, or float32 / float64 ``[P, 3]`` points (any row stride) that are
    quantised by ``voxel_size`` under ``rule``; ``rows`` int64 ``[E]`` or None: the points to take, in this order.
    -> ``coords`` int32 ``[U, 3]`` ascending lexicographically, ``inverse`` int64 ``[E]``, ``first`` int64 ``[U]`` (the
    smallest position of each voxel), ``counts`` int64 ``[U]`` and, with ``return_points``, ``coords * voxel_size`` in the
    points' type (float32 for coordinates).  The outputs are views of ``E``-row tensors."""
    who = "voxel_unique"
    src = _point_source(who, points_or_coords, rows, rule, True, voxel_size, size_optional=not return_points)
    return _unique(who, src, voxel_size, rule, return_points, _flags)


@torch.no_grad()
def quantise(points, voxel_size, rule="divide"):
    """float32 / float64 ``[P, 3]`` (any row stride) -> int32 ``[P, 3]``: ``torch.round(points / voxel_size).int()`` under
    the stated rule (``bsr_voxel_quantise``); a row that does not fit an int32 becomes ``(0, 0, 0)``.  No host read."""
    who = "quantise"
    src = _point_source(who, points, None, rule, False, voxel_size)
    return _quantise(src, float(voxel_size), rule)


@torch.no_grad()
def voxelize(points, voxel_size):
    """GM:435-438 on the device: float32 / float64 ``[P, 3]`` on the GPU -> the voxel centres ``[U, 3]`` in the points'
    type, rule ``divide``, rows in ``np.unique``'s order.  (What ``create_from_pcd`` calls between its two ``distCUDA2``.)"""
    who = "voxelize"
    src = _point_source(who, points, None, "divide", False, voxel_size)
    return _unique(who, src, float(voxel_size), "divide", True)[4]


def voxelize_sample(data, voxel_size):
    """Drop-in for ``GaussianModel.voxelize_sample`` (GM:435-438): ``np.unique(np.round(data / voxel_size), axis=0) *
    voxel_size`` for a numpy array (float64 or float32) or a tensor, returned as the same kind of object.  The data is
    uploaded once and quantised in its own type.  GM:436's shuffle is dropped: a unique does not depend on it."""
    who = "voxelize_sample"
    if isinstance(data, np.ndarray):
        if data.dtype not in (np.float32, np.float64):
            raise TypeError(f"{who}: data must be float32 or float64 (got {data.dtype})")
        if data.ndim != 2 or data.shape[1] != 3:
            raise ValueError(f"{who}: data must be [n, 3] (got {list(data.shape)})")
        _check_size(who, voxel_size)
        if not torch.cuda.is_available():
            raise ValueError(f"{who}: needs the GPU (there is no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device())
        return voxelize(torch.from_numpy(np.ascontiguousarray(data)).to(dev), voxel_size).cpu().numpy()
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"{who}: data must be a numpy array or a torch.Tensor (got {type(data).__name__})")
    if data.device.type == "cuda":
        return voxelize(data, voxel_size)
    if data.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: data must be float32 or float64 (got {data.dtype})")
    if data.dim() != 2 or data.shape[1] != 3:
        raise ValueError(f"{who}: data must be [n, 3] (got {list(data.shape)})")
    _check_size(who, voxel_size)
    if not torch.cuda.is_available():
        raise ValueError(f"{who}: needs the GPU (there is no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    return voxelize(data.to(dev), voxel_size).to(data.device)


@torch.no_grad()
def grow_level(anchor, offset, scaling, candidate_mask, anchor_feat, cur_size):
    """GM:824-862 of one ``anchor_growing`` level without the ``[N * K, 3]`` tensor of GM:824, its gathered copy and
    ``torch.unique``: the candidates' positions ``anchor[j // K] + offset[j] * scaling[j // K, :3]`` are formed, quantised
    (rule ``reciprocal``: what the GM lines compute on the GPU) and made unique in one native call.

    ``anchor`` float32 ``[N, 3]``; ``offset`` float32 ``[N, K, 3]`` or ``[N * K, 3]``; ``scaling`` float32 ``[N, >= 3]``
    (``get_scaling``'s ``[N, 6]`` is read in place); ``candidate_mask`` bool ``[N * K]``; ``anchor_feat`` float32
    ``[N, F]``; ``cur_size`` the level's voxel size.  -> ``candidate_anchor`` float32 ``[M, 3]`` and ``new_feat`` float32
    ``[M, F]`` as ``densify.grow_candidates`` returns them; no candidates: two empty tensors."""
    from .densify import scatter_max, voxel_isin
    who = "grow_level"
    tensors = (("anchor", anchor), ("offset", offset), ("scaling", scaling), ("anchor_feat", anchor_feat))
    mask = (("candidate_mask", candidate_mask),)
    _ops.check_tensors(who, tensors + mask, None)     # (every operand a tensor before any dtype is looked at)
    _ops.check_tensors(who, tensors, half_note=False)
    _ops.check_tensors(who, mask, torch.bool)
    if anchor.dim() != 2 or anchor.shape[1] != 3:
        raise ValueError(f"{who}: anchor must be [N, 3] (got {list(anchor.shape)})")
    N = anchor.shape[0]
    flat = offset.reshape(-1, 3) if offset.dim() in (2, 3) and offset.shape[-1] == 3 else None
    if flat is None or N == 0 or flat.shape[0] % N != 0 or flat.shape[0] == 0:
        raise ValueError(f"{who}: offset must hold K offsets for each of the {N} anchors (got {list(offset.shape)})")
    K = flat.shape[0] // N
    if scaling.dim() != 2 or scaling.shape[0] != N or scaling.shape[1] < 3:
        raise ValueError(f"{who}: scaling must be [{N}, >= 3] (got {list(scaling.shape)})")
    if anchor_feat.dim() != 2 or anchor_feat.shape[0] != N:
        raise ValueError(f"{who}: anchor_feat must be [{N}, F] (got {list(anchor_feat.shape)})")
    if tuple(candidate_mask.shape) != (N * K,):
        raise ValueError(f"{who}: candidate_mask must be [{N * K}] (got {list(candidate_mask.shape)})")
    if N * K >= 2 ** 31:
        raise ValueError(f"{who}: need N * K below 2^31 (got {N} * {K})")
    cur_size = _check_size(who, cur_size)
    _ops.check_on_gpu(who, tensors + mask)
    F = anchor_feat.shape[1]
    anchor, flat = anchor.detach().contiguous(), flat.detach().contiguous()
    scaling, scaling_stride = _strided_rows(scaling.detach())
    rows = candidate_mask.nonzero().squeeze(1)                                           # flat offset numbers
    empty = (torch.empty(0, 3, dtype=torch.float32, device=anchor.device),
             torch.empty(0, F, dtype=torch.float32, device=anchor.device))
    if rows.shape[0] == 0:
        return empty
    src = _Source(FORM_COMPOSITE, N * K, flat, 3, anchor, scaling, scaling_stride, K, rows)
    unique_coords, inverse, _, _ = _unique(who, src, cur_size, "reciprocal", False)      # GM:824, 831-834
    grid_coords = _quantise(_Source(FORM_POINTS_F, N, anchor), cur_size, "reciprocal")   # GM:829
    keep = ~voxel_isin(unique_coords, grid_coords)                                       # GM:838-849
    candidate_anchor = unique_coords[keep] * cur_size                                    # GM:850
    if candidate_anchor.shape[0] == 0:
        return empty
    out, _ = scatter_max(anchor_feat, inverse, unique_coords.shape[0], row_map=rows // K)   # GM:861-862
    return candidate_anchor, out[keep]
