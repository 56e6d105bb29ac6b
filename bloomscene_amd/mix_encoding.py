"""The context encoding ``pc.calc_interp_feat(anchor)`` on the MI355X: the normalisation by the anchor bounds
(``scene/gaussian_model.py:413-419``), ``mix_3D2D_encoding.forward`` (``:98-105``) over its four ``GridEncoder`` tables and
``STE_binary`` (``utils/encodings.py:177-192``, applied to the whole table by ``GridEncoder.forward``, ``:417-418``), fused
in HIP behind ``include/bloomscene_mix_grid.h``.

    out = mix_encode(x, tables, dims, bound_min=None, bound_max=None, binary=True)      # [n, F * sum L_g]
    out, dy_dx = mix_encode_maps(x, tables, dims, bound_min, bound_max, binary)         # measurement, no gradient
    enc = MixEncoding(n_features, resolutions_list, log2_hashmap_size, resolutions_list_2D, log2_hashmap_size_2D)
    features = enc(x, pc.x_bound_min, pc.x_bound_max)                                   # replaces gaussian_model.py:416-418

``x [n, 3]`` is read in place through its row stride; ``tables`` is a list of ``(params [rows, F], offsets [L + 1] int32,
resolutions [L] int32)``, the table layout of ``GridEncoder``; ``dims`` gives each table's coordinates, ascending indices
into (x, y, z) (``MIX_DIMS`` is the reference's mix).  No binary table is materialised: a corner reads the parameter and
takes its sign, so the result is bit-equal to ``grid_encode`` on ``STE_binary``'s output, and the output is written once
as ``[n, C]``.  One forward launch for all grids; the backward sums every table gradient in 64-bit fixed point (bit-identical
on every run, the rule of ``include/bloomscene_grid.h``) and applies ``STE_binary``'s gate in the pass that writes it.  An
unused ``x`` gradient costs neither ``dy_dx`` nor the input pass; frozen tables cost neither the contribution pass nor the
scratch.  The bounds are device tensors, never read on the host (the reference's host assert is gone): everything runs on
the current torch stream without a host synchronisation, capturable into a CUDA graph.  There is no CPU path; importing
this module needs no GPU.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from . import _operands as _ops
from ._operands import ptr, row_stride
from .grid_encoder import SUPPORTED_FEATURES, GridEncoder

MAX_GRIDS = 4      # BSR_MIX_MAX_GRIDS
MAX_LEVELS = 64    # over all grids
MIX_DIMS = ((0, 1, 2), (0, 1), (0, 2), (1, 2))   # scene/gaussian_model.py:100-103: xyz, xy, xz, yz


class _Grids:
    """The host arrays of ``include/bloomscene_mix_grid.h`` for one call (they keep their tensors alive)."""

    def __init__(self, params, offsets, resolutions, dims):
        G = self.G = len(params)
        self.tensors = (params, offsets, resolutions)
        pointers = lambda ts: (C.c_void_p * G)(*[t.data_ptr() or None for t in ts])
        ints = lambda vs: (C.c_int * len(vs))(*vs)
        self.params, self.offsets, self.resolutions = pointers(params), pointers(offsets), pointers(resolutions)
        self.levels = [int(r.shape[0]) for r in resolutions]
        self.rows = [int(p.shape[0]) for p in params]
        self.n_levels, self.n_rows = ints(self.levels), ints(self.rows)
        self.n_dims = ints([len(d) for d in dims])
        self.dims = ints([(list(d) + [0, 0, 0])[k] for d in dims for k in range(3)])
        self.F = int(params[0].shape[1])
        self.total_levels = sum(self.levels)
        self.C = self.F * self.total_levels
        self.W = self.F * sum(L * len(d) for L, d in zip(self.levels, dims))

    def args(self):
        return (self.params, self.offsets, self.resolutions, self.n_levels, self.n_rows, self.n_dims, self.dims)


class _MixEncode(torch.autograd.Function):
    """inputs: x, the two bounds (or None), binary, need_dx, want_maps, dims, the offsets and resolutions lists, the tables."""

    @staticmethod
    def forward(ctx, x, bmin, bmax, binary, need_dx, want_maps, dims, offsets, resolutions, *params):
        grids = _Grids(params, offsets, resolutions, dims)
        n, dev = x.shape[0], x.device
        out = torch.empty(n, grids.C, dtype=torch.float32, device=dev)
        dy_dx = torch.empty(n, grids.W, dtype=torch.float32, device=dev) if (need_dx or want_maps) else None
        if n > 0 and grids.C > 0:
            _capi.call("bsr_mix_grid_forward", n, grids.G, grids.F, int(binary), ptr(x), row_stride(x, n, 3), ptr(bmin),
                       ptr(bmax), *grids.args(), ptr(out), ptr(dy_dx), _ops.stream(dev))
        ctx.save_for_backward(x, bmin, bmax, dy_dx if need_dx else None, *params)
        ctx.mix = (bool(binary), dims, offsets, resolutions)
        if want_maps:
            ctx.mark_non_differentiable(dy_dx)
            return out, dy_dx
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, *_):
        x, bmin, bmax, dy_dx = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:]
        binary, dims, offsets, resolutions = ctx.mix
        need = ctx.needs_input_grad
        grids = _Grids(params, offsets, resolutions, dims)
        n, dev = x.shape[0], x.device
        d_x, d_params = None, [None] * grids.G
        if g_out is not None:
            g = g_out if g_out.dtype == torch.float32 else g_out.float()
            g = _ops.rows_in_place(g, n, grids.C)
            want = [bool(need[9 + k]) for k in range(grids.G)]
            new = torch.zeros if (n == 0 or grids.C == 0) else torch.empty
            d_params = [new(p.shape, dtype=torch.float32, device=dev) if w else None for p, w in zip(params, want)]
            if need[0] and dy_dx is not None:
                d_x = torch.empty(n, 3, dtype=torch.float32, device=dev)
            if n > 0 and grids.C > 0 and (any(want) or d_x is not None):
                scratch = None
                if any(want):
                    rows = (C.c_int * grids.G)(*[r if w else 0 for r, w in zip(grids.rows, want)])
                    scratch = _ops.scratch(_capi.lib().bsr_mix_grid_backward_scratch_bytes(grids.G, rows, grids.F,
                                                                                           grids.total_levels), dev)
                grads = (C.c_void_p * grids.G)(*[ptr(t) for t in d_params])
                _capi.call("bsr_mix_grid_backward", n, grids.G, grids.F, int(binary), ptr(g), row_stride(g, n, grids.C),
                           ptr(x), row_stride(x, n, 3), ptr(bmin), ptr(bmax), *grids.args(), ptr(dy_dx), grads,
                           ptr(d_x), ptr(scratch), _ops.stream(dev))
        return (d_x, None, None, None, None, None, None, None, None, *d_params)


def _checked(who, x, tables, dims, bound_min, bound_max):
    """The header's operands from the caller's tensors, checked in ``_operands``' order of complaints."""
    try:
        tables = [tuple(t) for t in tables]
        dims = tuple(tuple(int(k) for k in d) for d in dims)
        if any(len(t) != 3 for t in tables):
            raise TypeError
    except TypeError:
        raise ValueError(f"{who}: tables must be a list of (params, offsets, resolutions) and dims a list of index "
                         "tuples") from None
    floats = [("x", x)] + [(f"tables[{g}] params", t[0]) for g, t in enumerate(tables)]
    floats += [(name, b) for name, b in (("bound_min", bound_min), ("bound_max", bound_max)) if b is not None]
    ints = [(f"tables[{g}] {name}", t[k]) for g, t in enumerate(tables) for k, name in ((1, "offsets"), (2, "resolutions"))]
    _ops.check_tensors(who, floats + ints, None)     # (every operand a tensor before any dtype is looked at)
    _ops.check_tensors(who, floats)
    _ops.check_tensors(who, ints, torch.int32)
    if torch.is_grad_enabled():
        for name, b in (("bound_min", bound_min), ("bound_max", bound_max)):
            if b is not None and b.requires_grad:
                raise NotImplementedError(f"{who}: {name} requires a gradient; the encoding gives none to the bounds")
    if (bound_min is None) != (bound_max is None):
        raise ValueError(f"{who}: bound_min and bound_max come together")
    if not 1 <= len(tables) <= MAX_GRIDS:
        raise ValueError(f"{who}: 1 to {MAX_GRIDS} tables (got {len(tables)})")
    if len(dims) != len(tables):
        raise ValueError(f"{who}: one dims entry per table (got {len(dims)} for {len(tables)} tables)")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: x must be [n, 3] (got {list(x.shape)})")
    for name, b in (("bound_min", bound_min), ("bound_max", bound_max)):
        if b is not None and tuple(b.shape) not in ((3,), (1, 3)):
            raise ValueError(f"{who}: {name} must be [3] or [1, 3] (got {list(b.shape)})")
    F = None
    for g, ((p, o, r), d) in enumerate(zip(tables, dims)):
        if not 1 <= len(d) <= 3 or any(k < 0 or k > 2 for k in d) or any(a >= b for a, b in zip(d, d[1:])):
            raise ValueError(f"{who}: dims[{g}] must be 1 to 3 distinct ascending indices into (x, y, z) (got {d})")
        if p.dim() != 2 or p.shape[1] not in SUPPORTED_FEATURES:
            raise ValueError(f"{who}: tables[{g}] params must be [rows, F] with F in {SUPPORTED_FEATURES} (got {list(p.shape)})")
        if F is not None and p.shape[1] != F:
            raise ValueError(f"{who}: every table has the same F (tables[{g}] has {p.shape[1]}, tables[0] has {F})")
        F = p.shape[1]
        if o.dim() != 1 or r.dim() != 1 or o.shape[0] != r.shape[0] + 1:
            raise ValueError(f"{who}: tables[{g}] needs offsets [L + 1] and resolutions [L] (got {list(o.shape)}, {list(r.shape)})")
    levels = sum(int(t[2].shape[0]) for t in tables)
    if levels > MAX_LEVELS:
        raise ValueError(f"{who}: at most {MAX_LEVELS} levels over all tables (got {levels})")
    if x.shape[0] * F * levels >= 2 ** 31:
        raise ValueError(f"{who}: n * F * (levels of all tables) must be below 2^31 (got n = {x.shape[0]})")
    _ops.check_on_gpu(who, floats + ints)
    _ops.check_same_device(who, floats + ints, x.device)
    x = _ops.rows_in_place(x, x.shape[0], 3)
    params = [p if p.is_contiguous() else p.contiguous() for p, _, _ in tables]
    offsets = [o.detach().contiguous() for _, o, _ in tables]
    resolutions = [r.detach().contiguous() for _, _, r in tables]
    bounds = [None if b is None else b.detach().reshape(3).contiguous() for b in (bound_min, bound_max)]
    return x, params, offsets, resolutions, dims, bounds


def mix_encode(x, tables, dims, bound_min=None, bound_max=None, binary=True):
    """``x [n, 3]`` -> ``[n, F * sum L_g]``: every table of ``tables`` = ``[(params, offsets, resolutions), ...]`` encoded on
    its coordinates ``dims[g]`` of ``(x - bound_min) / (bound_max - bound_min)`` (``x`` itself without bounds), columns
    grid-major, then level, then channel.  ``binary``: a corner reads sign(p) (``STE_binary``), else p.  One autograd node,
    differentiable in ``x`` and every ``params``."""
    x, params, offsets, resolutions, dims, (bmin, bmax) = _checked("mix_encode", x, tables, dims, bound_min, bound_max)
    need_dx = torch.is_grad_enabled() and x.requires_grad
    return _MixEncode.apply(x, bmin, bmax, bool(binary), need_dx, False, dims, offsets, resolutions, *params)


@torch.no_grad()
def mix_encode_maps(x, tables, dims, bound_min=None, bound_max=None, binary=True):
    """``mix_encode`` and the saved ``dy_dx [n, F * sum L_g D_g]`` (per row, grid g's ``[L_g, D_g, F]`` block), for
    measurement (no gradient)."""
    x, params, offsets, resolutions, dims, (bmin, bmax) = _checked("mix_encode_maps", x, tables, dims, bound_min, bound_max)
    return _MixEncode.apply(x, bmin, bmax, bool(binary), False, True, dims, offsets, resolutions, *params)


class MixEncoding(nn.Module):
    """``mix_3D2D_encoding`` (``scene/gaussian_model.py:39-105``) with the reference's constructor arguments and submodule
    names -- ``encoding_xyz``, ``encoding_xy``, ``encoding_xz``, ``encoding_yz``, each a ``GridEncoder`` holding ``params``,
    ``offsets_list`` and ``resolutions_list`` -- so that a reference checkpoint's state dict loads key for key.
    ``forward(x, bound_min=None, bound_max=None)``: ``x [..., 3]`` -> ``[..., output_dim]``, the whole of
    ``calc_interp_feat`` in one autograd node."""

    NAMES = ("encoding_xyz", "encoding_xy", "encoding_xz", "encoding_yz")

    def __init__(self, n_features, resolutions_list, log2_hashmap_size, resolutions_list_2D, log2_hashmap_size_2D,
                 ste_binary=True, ste_multistep=False, add_noise=False, Q=1):
        super().__init__()
        if ste_multistep:
            raise NotImplementedError("MixEncoding: ste_multistep is not supported (include/bloomscene_mix_grid.h)")
        if add_noise:
            raise NotImplementedError("MixEncoding: add_noise is not supported (include/bloomscene_mix_grid.h)")
        self.ste_binary, self.Q = bool(ste_binary), Q
        self.encoding_xyz = GridEncoder(3, n_features, tuple(resolutions_list), log2_hashmap_size)
        for name in self.NAMES[1:]:
            setattr(self, name, GridEncoder(2, n_features, tuple(resolutions_list_2D), log2_hashmap_size_2D))
        self.output_dim = sum(getattr(self, name).output_dim for name in self.NAMES)

    def tables(self):
        return [(e.params, e.offsets_list, e.resolutions_list) for e in (getattr(self, name) for name in self.NAMES)]

    def forward(self, x, bound_min=None, bound_max=None):
        prefix = list(x.shape[:-1])
        out = mix_encode(x.reshape(-1, x.shape[-1]), self.tables(), MIX_DIMS, bound_min, bound_max, self.ste_binary)
        return out.view(prefix + [self.output_dim])
