"""``GaussianModel.adjust_anchor`` (``scene/gaussian_model.py:898-952``, "GM", with ``anchor_growing`` GM:807-895,
``cat_tensors_to_optimizer`` GM:719-740 and ``_prune_anchor_optimizer`` GM:761-791) on the MI355X, in HIP behind
``include/bloomscene_adjust.h``, which states the function.

    bloomscene_amd.adjust.adjust_anchor(self.gaussians, check_interval=..., success_threshold=..., grad_threshold=...,
                                        min_opacity=...)          # for self.gaussians.adjust_anchor(...) at bloomscene.py:349

    offset_flags, anchor_flags, src_of, status = decide(opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, K,
                                                        thresholds, check_interval, success_threshold, min_opacity)
    new_tensors                                = resize_rows(tensors, src_of, n_keep, appends, fills, ops)
    blocks                                     = grow(model, offset_flags, rand)
    quantize_anchor(x, bound_min, bound_max)   # the 16-bit lattice of get_anchor, in eager torch
    resize_optimizer(optimizer, new_params_by_name, new_moments_by_name)

Each per-anchor tensor of the result is the kept old rows in ascending order followed by the new rows in level order:
``decide`` is one launch chain over the four statistics and makes no host read, ``adjust_anchor`` reads the new row count
once, and ONE ``resize_rows`` call writes every parameter, moment and statistic exactly once.

Deviations from the reference.  (1) The reference draws ``N_i * K`` random numbers at level ``i`` (``N_i`` grows with the
anchors of the earlier levels, which are never candidates); here every level draws ``N * K``.  The random stream differs,
the distribution of every decision does not, and with the same ``rand`` tensors the results are equal bit for bit.  (2) The
old and the new copy of all per-anchor state are alive together during the one launch (about 1.1 KB an anchor for F = 32,
K = 10); the reference holds one tensor's pair at a time.

Everything runs on the current torch stream with memory from torch's allocator.  There is no CPU path; importing this
module needs no GPU.
"""
from __future__ import annotations

import struct

import torch

from . import _capi
from . import _operands as _ops
from ._capi import ResizeTensor

__all__ = ["decide", "resize_rows", "quantize_anchor", "grow", "resize_optimizer", "adjust_anchor"]

# include/bloomscene_adjust.h
RESIZE_COPY, RESIZE_ZERO_FLAGGED, RESIZE_CLAMP_FROM = 0, 1, 2
MAX_K, MAX_LEVELS, MAX_WIDTH = 16, 7, 1024
OFFSET_VALID, ANCHOR_PRUNE, ANCHOR_VALID = 0x80, 0x01, 0x02

SKIPPED_GROUPS = ("mlp", "conv", "feat_base", "encoding")                       # GM:722, 764
ATTRIBUTE_OF_GROUP = {"anchor": "_anchor", "offset": "_offset", "mask": "_mask", "anchor_feat": "_anchor_feat",
                      "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
SCALING_CLAMP_COL, SCALING_CLAMP = 3, 0.05                                       # GM:775-779


def _raise_in_order(who, wrong_type, unsupported, wrong_shape, wrong_device):
    """The first finding, in ``_operands``' order of complaints."""
    for kind, finding in ((TypeError, wrong_type), (NotImplementedError, unsupported), (ValueError, wrong_shape),
                          (ValueError, wrong_device)):
        if finding:
            raise kind(f"{who}: {finding}")


def _check_tensors(named, dtypes):
    """-> the first dtype finding (TypeError) of [(name, tensor)], in ``_operands``' words."""
    return _ops.wrong_tensor(named, dtypes, half_note=False)


# ---- A ----

@torch.no_grad()
def decide(opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, K, thresholds, check_interval=100,
           success_threshold=0.8, min_opacity=0.005):
    """The decisions of GM:900-903, 811-812 and 921-923 and the plan (``bsr_adjust_decide``).

    The statistics are float32 ``[N]`` / ``[N, 1]`` (per anchor) and ``[N * K]`` / ``[N * K, 1]`` (per offset);
    ``thresholds`` is a sequence of 1 to 7 python floats, level ``i``'s ``grad_threshold * ((update_hierachy_factor // 2)
    ** i)``.  -> ``offset_flags`` uint8 ``[N * K]`` (bit ``i``: a candidate of level ``i`` before the random mask; bit 7:
    the offset's statistics are reset), ``anchor_flags`` uint8 ``[N]`` (bit 0: pruned, bit 1: statistics reset), ``src_of``
    int32 ``[N]`` (its first ``n_keep`` entries: the kept rows, ascending) and ``status`` int32 ``[4]`` ``{n_keep, anchors
    reset, offsets reset, 0}``, which stays on the device: no host read."""
    who = "decide"
    named = (("opacity_accum", opacity_accum), ("anchor_demon", anchor_demon),
             ("offset_gradient_accum", offset_gradient_accum), ("offset_denom", offset_denom))
    wrong_type = _check_tensors(named, (torch.float32,))
    if wrong_type is None and (isinstance(K, bool) or not isinstance(K, int)):
        wrong_type = f"K must be an int (got {type(K).__name__})"
    _raise_in_order(who, wrong_type, None, None, None)
    thresholds = [float(t) for t in thresholds]
    wrong_shape = None
    if not 1 <= K <= MAX_K:
        wrong_shape = f"K must be in [1, {MAX_K}] (got {K})"
    elif not 1 <= len(thresholds) <= MAX_LEVELS:
        wrong_shape = f"need 1 to {MAX_LEVELS} thresholds (got {len(thresholds)})"
    else:
        N = opacity_accum.numel()
        for (name, t), want in zip(named, (N, N, N * K, N * K)):
            if t.numel() != want or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
                wrong_shape = wrong_shape or f"{name} must be [{want}] or [{want}, 1] (got {list(t.shape)})"
        if N * K >= 2 ** 31:
            wrong_shape = wrong_shape or f"need N * K below 2^31 (got {N} * {K})"
    _raise_in_order(who, None, None, wrong_shape, _ops.off_gpu(named))
    dev = opacity_accum.device
    stats = [t.detach().reshape(-1).contiguous() for _, t in named]
    offset_flags = torch.empty(N * K, dtype=torch.uint8, device=dev)
    anchor_flags = torch.empty(N, dtype=torch.uint8, device=dev)
    src_of = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return offset_flags, anchor_flags, src_of, torch.zeros(4, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    scratch = _ops.scratch(_capi.lib().bsr_adjust_decide_scratch_bytes(N), dev)
    thr = (_capi.C.c_double * len(thresholds))(*thresholds)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _capi.call("bsr_adjust_decide", N, K, *[ptr(t) for t in stats], len(thresholds), thr,
               check_interval * success_threshold * 0.5, check_interval * success_threshold, float(min_opacity),
               ptr(offset_flags), ptr(anchor_flags), ptr(src_of), status.data_ptr(), ptr(scratch), _ops.stream(dev))
    return offset_flags, anchor_flags, src_of, status


# ---- B ----

def _fill_bits(fill, dtype):
    if fill is None:
        return 0
    if dtype == torch.int32:
        return int(fill) & 0xffffffff
    return struct.unpack("<I", struct.pack("<f", float(fill)))[0]


@torch.no_grad()
def resize_rows(tensors, src_of, n_keep, appends=None, fills=None, ops=None, n_append=None, out=None):
    """Prune and append the rows of many tensors in one native call (``bsr_rows_resize``).

    ``tensors``  float32 or int32 tensors with the same number ``N`` of rows (dimension 0); a row is at most 1024 elements
    ``src_of``   int32 ``[>= n_keep]`` on the GPU: row ``i < n_keep`` of every result is row ``src_of[i]`` of its tensor
                 (an entry outside ``[0, N)`` gives a row of zeros)
    ``appends``  None, or per tensor None or the ``A`` rows that follow the kept ones (the tensor's own type and row shape)
    ``fills``    None, or per tensor None (0) or the number every appended element is where the tensor has no ``appends``
    ``ops``      None, or per tensor None, ``("zero_flagged", flags, mask, per_element)`` -- a kept element whose uint8
                 flag (``flags[row]``, or ``flags[row * width + column]`` with ``per_element``) has a bit of ``mask``
                 becomes +0 -- or ``("clamp_from", column, bound)``: ``v > bound ? bound : v`` from that column on, in
                 kept and appended rows
    ``n_append`` ``A`` where no tensor has ``appends`` (default 0)
    ``out``      None, or per tensor a contiguous tensor of ``(n_keep + A) * width`` elements to write instead of a new one
    -> the new tensors ``[n_keep + A, ...]``, each written exactly once.  No host read."""
    who = "resize_rows"
    tensors = list(tensors)
    n = len(tensors)
    appends = list(appends) if appends is not None else [None] * n
    fills = list(fills) if fills is not None else [None] * n
    ops = list(ops) if ops is not None else [None] * n
    outs = list(out) if out is not None else [None] * n
    both = (torch.float32, torch.int32)
    wrong_type = _check_tensors([(f"tensors[{i}]", t) for i, t in enumerate(tensors)], both)
    wrong_type = wrong_type or _check_tensors([("src_of", src_of)], (torch.int32,))
    flag_tensors = [(f"ops[{i}]: flags", op[1]) for i, op in enumerate(ops) if op is not None and op[0] == "zero_flagged"]
    wrong_type = wrong_type or _check_tensors(flag_tensors, (torch.uint8,))
    for i, (t, a, o) in enumerate(zip(tensors, appends, outs)):
        for name, x in ((f"appends[{i}]", a), (f"out[{i}]", o)):
            if x is not None and wrong_type is None:
                wrong_type = _check_tensors([(name, x)], (t.dtype,)) if isinstance(t, torch.Tensor) else None
    _raise_in_order(who, wrong_type, None, None, None)
    wrong_shape = None
    if not (len(appends) == len(fills) == len(ops) == len(outs) == n):
        wrong_shape = f"appends, fills, ops and out must have one entry per tensor ({n})"
    _raise_in_order(who, None, None, wrong_shape, None)
    A = None if n_append is None else int(n_append)
    for a in appends:
        if a is not None:
            if A is not None and a.shape[0] != A:
                wrong_shape = wrong_shape or f"the appends must have the same number of rows (got {a.shape[0]} and {A})"
            A = a.shape[0]
    A = A or 0
    n_keep = int(n_keep)
    N = tensors[0].shape[0] if n and tensors[0].dim() else 0
    widths = []
    for i, (t, a, op, o) in enumerate(zip(tensors, appends, ops, outs)):
        if t.dim() == 0 or t.shape[0] != N:
            wrong_shape = wrong_shape or f"tensors[{i}] must have {N} rows (got {list(t.shape)})"
            widths.append(1)
            continue
        w = 1
        for s in t.shape[1:]:
            w *= s
        widths.append(w)
        if not 1 <= w <= MAX_WIDTH:
            wrong_shape = wrong_shape or f"tensors[{i}]: a row must be 1 to {MAX_WIDTH} elements (got {w})"
        if a is not None and tuple(a.shape[1:]) != tuple(t.shape[1:]):
            wrong_shape = wrong_shape or f"appends[{i}] must be [A, {list(t.shape[1:])}] (got {list(a.shape)})"
        if o is not None and (o.numel() != (n_keep + A) * w or not o.is_contiguous()):
            wrong_shape = wrong_shape or f"out[{i}] must be contiguous with {(n_keep + A) * w} elements (got {list(o.shape)})"
        if (n_keep + A) * w >= 2 ** 31:
            wrong_shape = wrong_shape or f"tensors[{i}]: need (n_keep + A) * width below 2^31"
        if op is not None:
            if op[0] == "zero_flagged":
                want = N * w if op[3] else N
                if op[1].numel() != want:
                    wrong_shape = wrong_shape or f"ops[{i}]: flags must have {want} elements (got {op[1].numel()})"
                if not 0 <= int(op[2]) <= 0xff:
                    wrong_shape = wrong_shape or f"ops[{i}]: mask must be in [0, 255] (got {op[2]})"
            elif op[0] == "clamp_from":
                if t.dtype != torch.float32 or not 0 <= int(op[1]) <= w:
                    wrong_shape = wrong_shape or f"ops[{i}]: clamp_from needs a float32 tensor and a column in [0, {w}]"
            else:
                wrong_shape = wrong_shape or f"ops[{i}]: unknown op {op[0]!r}"
    if not 0 <= n_keep <= N:
        wrong_shape = wrong_shape or f"n_keep must be in [0, {N}] (got {n_keep})"
    if A < 0:
        wrong_shape = wrong_shape or f"n_append must be >= 0 (got {A})"
    if src_of.dim() != 1 or src_of.shape[0] < n_keep:
        wrong_shape = wrong_shape or f"src_of must be [>= {n_keep}] (got {list(src_of.shape)})"
    on_device = [(f"tensors[{i}]", t) for i, t in enumerate(tensors)] + [("src_of", src_of)] + flag_tensors
    on_device += [(f"appends[{i}]", a) for i, a in enumerate(appends) if a is not None]
    on_device += [(f"out[{i}]", o) for i, o in enumerate(outs) if o is not None]
    _raise_in_order(who, None, None, wrong_shape, _ops.off_gpu(on_device))
    if n == 0:
        return []
    dev = tensors[0].device
    arr = (ResizeTensor * n)()
    keep, results = [], []
    for d, t, a, f, op, o, w in zip(arr, tensors, appends, fills, ops, outs, widths):
        src = t.detach().contiguous()
        dst = o if o is not None else torch.empty((n_keep + A,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        keep.append(src)
        d.src, d.dst, d.width = src.data_ptr() if src.numel() else None, dst.data_ptr() if dst.numel() else None, w
        if a is not None and A > 0:
            a = a.detach().contiguous()
            keep.append(a)
            d.append = a.data_ptr()
        else:
            d.append = None
        d.fill = _fill_bits(f, t.dtype)
        d.flags, d.flags_per_element, d.flag_mask, d.op, d.clamp_col, d.clamp = None, 0, 0, RESIZE_COPY, 0, 0.0
        if op is not None and op[0] == "zero_flagged":
            flags = op[1].contiguous()
            keep.append(flags)
            d.flags, d.flag_mask, d.flags_per_element = flags.data_ptr() if flags.numel() else None, int(op[2]), int(bool(op[3]))
            d.op = RESIZE_ZERO_FLAGGED
        elif op is not None:
            d.op, d.clamp_col, d.clamp = RESIZE_CLAMP_FROM, int(op[1]), float(op[2])
        results.append(dst)
    src_of = src_of.contiguous()
    _capi.call("bsr_rows_resize", n, arr, N, n_keep, A, src_of.data_ptr() if src_of.numel() else None, _ops.stream(dev))
    return results


# ---- C ----

@torch.no_grad()
def quantize_anchor(x, bound_min, bound_max):
    """The 16-bit lattice ``get_anchor`` puts ``_anchor`` on (GM:394-399), in eager torch, by the sequence
    ``include/bloomscene_anchor_state.h`` states: ``interval = (max - min) * fl32(1 / 65535) + fl32(1e-6)``,
    ``q = clamp(floor_divide(x - min, interval), 0, 65535)``, ``q * interval + min``."""
    interval = (bound_max - bound_min) * (1.0 / 65535.0) + 1e-6
    q = torch.clamp(torch.div(x - bound_min, interval, rounding_mode="floor"), 0, 65535)
    return q * interval + bound_min


@torch.no_grad()
def grow(model, offset_flags, rand):
    """The levels of ``anchor_growing`` (GM:807-895) without appending between levels.

    Level ``i``'s candidates are bit ``i`` of ``offset_flags`` and ``rand[i] > 0.5 ** (i + 1)`` over the OLD ``N * K``
    offsets (new anchors have zero statistics and are never candidates).  Its occupied voxels are those of
    ``model.get_anchor`` and of the anchors the earlier levels produced, taken through ``quantize_anchor`` as
    ``get_anchor`` does in the reference.  A level ``i > 0`` is skipped entirely while no earlier level has added an anchor
    (GM:819-821).  -> ``{"anchor": [A, 3], "scaling": [A, 6], "rotation": [A, 4], "anchor_feat": [A, F]}``, the appended
    blocks in level order; everything else of a new anchor is a constant."""
    from . import voxelize as V
    from .densify import scatter_max, voxel_isin
    who = "grow"
    wrong_type = _check_tensors([("offset_flags", offset_flags)], (torch.uint8,))
    wrong_type = wrong_type or _check_tensors([(f"rand[{i}]", r) for i, r in enumerate(rand)], (torch.float32,))
    _raise_in_order(who, wrong_type, None, None, None)
    K, depth = int(model.n_offsets), int(model.update_depth)
    N = model._anchor.shape[0]
    wrong_shape = None
    if len(rand) != depth:
        wrong_shape = f"need one rand tensor per level ({depth}, got {len(rand)})"
    for i, r in enumerate(rand):
        if r.numel() != N * K:
            wrong_shape = wrong_shape or f"rand[{i}] must have {N * K} elements (got {list(r.shape)})"
    if offset_flags.numel() != N * K:
        wrong_shape = wrong_shape or f"offset_flags must have {N * K} elements (got {list(offset_flags.shape)})"
    on_device = [("offset_flags", offset_flags)] + [("rand", r) for r in rand]
    _raise_in_order(who, None, None, wrong_shape, _ops.off_gpu(on_device))
    dev = offset_flags.device
    F = model._anchor_feat.shape[1]
    blocks = {"anchor": [], "scaling": [], "rotation": [], "anchor_feat": []}
    if N == 0:
        depth = 0
    else:
        anchor = model.get_anchor.detach().contiguous()
        flat = model._offset.detach().reshape(-1, 3).contiguous()
        scaling, scaling_stride = V._strided_rows(model.get_scaling.detach())
        feat = model._anchor_feat.detach()
    pending = []                                                               # the earlier levels' anchors, on the lattice
    for i in range(depth):
        if i > 0 and not pending:
            continue                                                           # GM:819-821
        candidate = ((offset_flags.reshape(-1) >> i) & 1).bool() & (rand[i].reshape(-1) > 0.5 ** (i + 1))    # GM:811-816
        cur_size = model.voxel_size * (model.update_init_factor // (model.update_hierachy_factor ** i))      # GM:826-827
        rows = candidate.nonzero().squeeze(1)
        if rows.shape[0] == 0:
            continue
        src = V._Source(V.FORM_COMPOSITE, N * K, flat, 3, anchor, scaling, scaling_stride, K, rows)
        unique_coords, inverse, _, _ = V._unique(who, src, cur_size, "reciprocal", False)                    # GM:824, 831-834
        occupied = torch.cat([anchor] + pending) if pending else anchor
        grid_coords = V.quantise(occupied, cur_size, "reciprocal")                                           # GM:829
        keep = ~voxel_isin(unique_coords, grid_coords)                                                       # GM:838-849
        candidate_anchor = unique_coords[keep] * cur_size                                                    # GM:850
        if candidate_anchor.shape[0] == 0:
            continue
        new_feat, _ = scatter_max(feat, inverse, unique_coords.shape[0], row_map=rows // K)                  # GM:861-862
        blocks["anchor"].append(candidate_anchor)
        blocks["scaling"].append(torch.log(torch.ones(candidate_anchor.shape[0], 6, device=dev) * cur_size))  # GM:853-854
        blocks["anchor_feat"].append(new_feat[keep])
        pending.append(quantize_anchor(candidate_anchor, model.x_bound_min, model.x_bound_max))
    A = sum(b.shape[0] for b in blocks["anchor"])
    rotation = torch.zeros(A, 4, device=dev)
    rotation[:, 0] = 1.0                                                                                     # GM:856-857
    empty = {"anchor": torch.empty(0, 3, device=dev), "scaling": torch.empty(0, 6, device=dev),
             "anchor_feat": torch.empty(0, F, device=dev)}
    out = {k: (torch.cat(v) if v else empty[k]) for k, v in blocks.items() if k != "rotation"}
    out["rotation"] = rotation
    return out


_OPACITY_FILL = {}


def _opacity_fill(dev):
    """inverse_sigmoid(0.1) as the device's torch forms it for GM:859, read once per device."""
    if dev not in _OPACITY_FILL:
        x = 0.1 * torch.ones(1, dtype=torch.float, device=dev)
        _OPACITY_FILL[dev] = float(torch.log(x / (1 - x)).item())
    return _OPACITY_FILL[dev]


def _is_skipped(name):
    return any(s in name for s in SKIPPED_GROUPS)


def resize_optimizer(optimizer, new_params_by_name, new_moments_by_name):
    """The re-keying of GM:711-713 for every per-anchor group, for ``torch.optim.Adam`` and ``bloomscene_amd.optim.Adam`` in
    both its forms: the group gets ``nn.Parameter(new_params_by_name[name])``; a group with state moves it to the new
    parameter with ``exp_avg``, ``exp_avg_sq = new_moments_by_name[name]`` and the inherited ``step`` (wherever it lives);
    a group without state gets no state.  Groups whose names contain ``mlp``, ``conv``, ``feat_base`` or ``encoding`` are
    left alone.  -> ``{name: the new parameter}``."""
    out = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name is None or _is_skipped(name) or name not in new_params_by_name:
            continue
        if len(group["params"]) != 1:
            raise ValueError(f"resize_optimizer: group {name!r} must hold one parameter (got {len(group['params'])})")
        old = group["params"][0]
        stored = optimizer.state.get(old, None)
        new = torch.nn.Parameter(new_params_by_name[name].requires_grad_(True))
        if stored:
            stored["exp_avg"], stored["exp_avg_sq"] = new_moments_by_name[name]
            del optimizer.state[old]
            optimizer.state[new] = stored
        elif old in optimizer.state:
            del optimizer.state[old]
        group["params"][0] = new
        out[name] = new
    return out


@torch.no_grad()
def adjust_anchor(model, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005, rand=None):
    """Drop-in for ``GaussianModel.adjust_anchor`` (GM:898-952) on a duck-typed model (the module docstring has the
    deviations).  ``rand``: None, or ``update_depth`` float32 tensors of ``N * K`` uniforms, level ``i``'s random mask being
    ``rand[i] > 0.5 ** (i + 1)``.  One host read (the new row count)."""
    who = "adjust_anchor"
    K, depth = int(model.n_offsets), int(model.update_depth)
    N = model._anchor.shape[0]
    dev = model._anchor.device
    thresholds = [grad_threshold * ((model.update_hierachy_factor // 2) ** i) for i in range(depth)]           # GM:810
    offset_flags, anchor_flags, src_of, status = decide(model.opacity_accum, model.anchor_demon, model.offset_gradient_accum,
                                                        model.offset_denom, K, thresholds, check_interval,
                                                        success_threshold, min_opacity)
    if rand is None:
        rand = [torch.rand(N * K, device=dev) for _ in range(depth)]
    n_keep = int(status[0].item())                                             # the call's one host read
    blocks = grow(model, offset_flags, rand)
    A = blocks["anchor"].shape[0]
    fill_of = {"offset": 0.0, "mask": 1.0, "opacity": _opacity_fill(dev)}       # GM:859, 865-866
    names, tensors, appends, fills, ops = [], [], [], [], []

    def add(name, t, append=None, fill=None, op=None):
        names.append(name)
        tensors.append(t)
        appends.append(append)
        fills.append(fill)
        ops.append(op)

    with_state = set()
    for group in model.optimizer.param_groups:
        name = group.get("name")
        if name is None or _is_skipped(name):
            continue
        if name not in ATTRIBUTE_OF_GROUP:
            raise ValueError(f"{who}: no per-anchor tensor is known for the optimizer group {name!r}")
        if len(group["params"]) != 1:
            raise ValueError(f"{who}: group {name!r} must hold one parameter (got {len(group['params'])})")
        p = group["params"][0]
        if p.shape[0] != N:
            raise ValueError(f"{who}: group {name!r} has {p.shape[0]} rows, the model {N} anchors")
        op = ("clamp_from", SCALING_CLAMP_COL, SCALING_CLAMP) if name == "scaling" else None
        add(name, p, blocks.get(name), fill_of.get(name), op)
        stored = model.optimizer.state.get(p, None)
        if stored:                                                             # GM:727-729, 768-770
            with_state.add(name)
            add(name + ".exp_avg", stored["exp_avg"])
            add(name + ".exp_avg_sq", stored["exp_avg_sq"])
    per_row = ("zero_flagged", anchor_flags, ANCHOR_VALID, False)              # GM:938-939
    per_offset = ("zero_flagged", offset_flags, OFFSET_VALID, True)            # GM:908, 914
    add("opacity_accum", model.opacity_accum.reshape(N, 1), op=per_row)
    add("anchor_demon", model.anchor_demon.reshape(N, 1), op=per_row)
    add("offset_gradient_accum", model.offset_gradient_accum.reshape(N, K), op=per_offset)
    add("offset_denom", model.offset_denom.reshape(N, K), op=per_offset)
    new = dict(zip(names, resize_rows(tensors, src_of, n_keep, appends, fills, ops, n_append=A)))
    params = {name: new[name] for name in names if name in ATTRIBUTE_OF_GROUP}
    moments = {name: (new[name + ".exp_avg"], new[name + ".exp_avg_sq"]) for name in with_state}
    for name, p in resize_optimizer(model.optimizer, params, moments).items():
        setattr(model, ATTRIBUTE_OF_GROUP[name], p)
    model.opacity_accum = new["opacity_accum"]
    model.anchor_demon = new["anchor_demon"]
    model.offset_gradient_accum = new["offset_gradient_accum"].view(-1, 1)
    model.offset_denom = new["offset_denom"].view(-1, 1)
    model.max_radii2D = torch.zeros(n_keep + A, device=dev)                    # GM:952
