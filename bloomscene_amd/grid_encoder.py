"""Multi-resolution hash-grid encoder on the MI355X: BloomScene's ``_gridencoder`` (``utils/encodings.py:230-349``,
``submodules/gridencoder``) restated in HIP behind ``include/bloomscene_grid.h``.

    out = grid_encode(inputs, embeddings, offsets, resolutions, min_level=0, n_levels=None)   # [N, n_levels * F]

``inputs [N, D]`` in [0, 1] (a point with a coordinate outside encodes to 0), ``embeddings [rows, F]`` (the whole
table), ``offsets [L + 1]`` / ``resolutions [L]`` int32 on the same device: the table layout of ``GridEncoder``.
Levels ``min_level .. min_level + n_levels - 1`` are computed (the reference's int ``min_level_id`` slicing).  The
output is level-major per point, like the reference's ``outputs.permute(1, 0, 2).reshape(N, L * F)``.

The gradient with respect to ``embeddings`` is summed in 64-bit fixed point with integer atomics: bit-identical on
every run (the reference's float ``atomicAdd`` is not); the rule and its error bound are in the header.  The gradient
with respect to ``inputs`` is the reference's ``dy_dx`` formula.  Everything runs on the current torch stream without a
host synchronisation (capturable into a CUDA graph).  There is no CPU path.  The quantisers BloomScene wraps around the
table (STE etc.) stay the caller's torch code here; ``bloomscene_amd.mix_encoding`` fuses ``STE_binary`` and the four
tables of ``mix_3D2D_encoding`` into one call.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _capi
from . import _operands as _ops
from ._operands import ptr

SUPPORTED_DIMS = (1, 2, 3)
SUPPORTED_FEATURES = (1, 2, 4, 8)


def check_call(who, num_dim, n_features, float_tensors=(), int_tensors=(), binary_vxl=None, min_level_id=None):
    """The checks every entry point makes before any native call, in an order of its own (``_operands`` states the
    wrappers'): unsupported reference options raise NotImplementedError, unsupported shapes ValueError, dtypes
    TypeError, tensors off the GPU ValueError."""
    if binary_vxl is not None:
        raise NotImplementedError(f"{who}: binary_vxl is not supported (include/bloomscene_grid.h)")
    if min_level_id is not None:
        raise NotImplementedError(f"{who}: a per-point min_level_id is not supported; slice offsets / resolutions "
                                  "for an int level offset")
    if num_dim not in SUPPORTED_DIMS:
        raise ValueError(f"{who}: num_dim must be one of {SUPPORTED_DIMS} (got {num_dim})")
    if n_features not in SUPPORTED_FEATURES:
        raise ValueError(f"{who}: n_features must be one of {SUPPORTED_FEATURES} (got {n_features})")
    for tensors, dtype in ((float_tensors, torch.float32), (int_tensors, torch.int32)):
        for name, t in tensors:
            if t is not None and t.dtype != dtype:
                raise TypeError(f"{who}: {_ops.dtype_complaint(name, t, dtype)}")
    for name, t in tuple(float_tensors) + tuple(int_tensors):
        if t is None:
            continue
        _ops.check_on_gpu(who, [(name, t)])
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")


def forward_into(inputs, embeddings, offsets, resolutions, outputs, dy_dx, n_levels):
    """bsr_grid_encode_forward on tensors already checked: outputs [L, N, F], dy_dx [N, L * D * F] or None."""
    N, D = inputs.shape
    F = embeddings.shape[1]
    _capi.call("bsr_grid_encode_forward", N, D, F, n_levels, embeddings.shape[0], ptr(inputs), ptr(embeddings),
               ptr(offsets), ptr(resolutions), ptr(outputs), ptr(dy_dx), _ops.stream(inputs.device))


def backward_into(grad, inputs, offsets, resolutions, grad_embeddings, dy_dx, grad_inputs, n_levels):
    """bsr_grid_encode_backward on tensors already checked: grad [L, N, F]; grad_embeddings fully overwritten; the
    scratch comes from torch's allocator."""
    N, D = inputs.shape
    rows, F = grad_embeddings.shape
    scratch = _ops.scratch(_capi.lib().bsr_grid_backward_scratch_bytes(rows, F, n_levels), inputs.device)
    _capi.call("bsr_grid_encode_backward", N, D, F, n_levels, rows, ptr(grad), ptr(inputs), ptr(offsets),
               ptr(resolutions), ptr(dy_dx), ptr(grad_embeddings), ptr(grad_inputs), ptr(scratch),
               _ops.stream(inputs.device))


class _GridEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, resolutions, min_level, n_levels):
        N, D = inputs.shape
        F = embeddings.shape[1]
        offs = offsets[min_level:min_level + n_levels + 1]
        res = resolutions[min_level:min_level + n_levels]
        outputs = torch.empty(n_levels, N, F, dtype=torch.float32, device=inputs.device)
        need_dx = ctx.needs_input_grad[0]
        dy_dx = torch.empty(N, n_levels * D * F, dtype=torch.float32, device=inputs.device) if need_dx else None
        forward_into(inputs, embeddings, offs, res, outputs, dy_dx, n_levels)
        ctx.save_for_backward(inputs, offs, res, dy_dx)
        ctx.shape = (N, D, F, n_levels, embeddings.shape[0])
        return outputs.permute(1, 0, 2).reshape(N, n_levels * F)

    @staticmethod
    def backward(ctx, grad):
        inputs, offs, res, dy_dx = ctx.saved_tensors
        N, D, F, L, rows = ctx.shape
        g = grad.view(N, L, F).permute(1, 0, 2).contiguous().float()
        grad_embeddings = torch.empty(rows, F, dtype=torch.float32, device=inputs.device)
        grad_inputs = torch.empty(N, D, dtype=torch.float32, device=inputs.device) if dy_dx is not None else None
        backward_into(g, inputs, offs, res, grad_embeddings, dy_dx, grad_inputs, L)
        return grad_inputs, grad_embeddings, None, None, None, None


def grid_encode(inputs, embeddings, offsets, resolutions, min_level=0, n_levels=None):
    """Encode ``inputs [N, D]`` on levels ``min_level .. min_level + n_levels - 1`` of the table -> ``[N, n_levels * F]``
    (differentiable in ``inputs`` and ``embeddings``)."""
    if not isinstance(min_level, int):
        raise NotImplementedError("grid_encode: min_level must be an int (a per-point level offset is not supported)")
    if inputs.dim() != 2 or embeddings.dim() != 2:
        raise ValueError("grid_encode: inputs must be [N, D] and embeddings [rows, F]")
    inputs = inputs.contiguous()
    D, F = inputs.shape[1], embeddings.shape[1]
    check_call("grid_encode", D, F, float_tensors=(("inputs", inputs), ("embeddings", embeddings)),
               int_tensors=(("offsets", offsets), ("resolutions", resolutions)))
    L_all = resolutions.shape[0]
    if n_levels is None:
        n_levels = L_all - min_level
    if min_level < 0 or n_levels < 0 or min_level + n_levels > L_all or offsets.shape[0] != L_all + 1:
        raise ValueError(f"grid_encode: levels {min_level} .. {min_level + n_levels - 1} of a {L_all}-level table "
                         f"({offsets.shape[0]} offsets)")
    return _GridEncode.apply(inputs, embeddings, offsets, resolutions, min_level, n_levels)


def level_rows(num_dim, resolutions, log2_hashmap_size):
    """Rows of each level: min(2^log2_hashmap_size, res^D) rounded up to a multiple of 8 (the reference's rule,
    utils/encodings.py:386-391)."""
    cap = 2 ** log2_hashmap_size
    return [int(np.ceil(min(cap, int(r) ** num_dim) / 8) * 8) for r in resolutions]


def table_offsets(num_dim, resolutions, log2_hashmap_size):
    """[L + 1] first row of each level, then the total."""
    return [0] + np.cumsum(level_rows(num_dim, resolutions, log2_hashmap_size)).tolist()


class GridEncoder(nn.Module):
    """The table of BloomScene's ``GridEncoder`` (offsets, resolutions, ``params [rows, F]``) with the encode on the
    MI355X.  ``forward(inputs, min_level=0, n_levels=None)``: ``inputs [..., D]`` -> ``[..., n_levels * F]``."""

    def __init__(self, num_dim=3, n_features=2, resolutions=(16, 23, 32, 46, 64, 92, 128, 184, 256, 368, 512, 736),
                 log2_hashmap_size=19):
        super().__init__()
        if num_dim not in SUPPORTED_DIMS:
            raise ValueError(f"GridEncoder: num_dim must be one of {SUPPORTED_DIMS} (got {num_dim})")
        if n_features not in SUPPORTED_FEATURES:
            raise ValueError(f"GridEncoder: n_features must be one of {SUPPORTED_FEATURES} (got {n_features})")
        self.num_dim, self.n_features, self.log2_hashmap_size = num_dim, n_features, log2_hashmap_size
        self.n_levels = len(resolutions)
        self.output_dim = self.n_levels * n_features
        offsets = table_offsets(num_dim, resolutions, log2_hashmap_size)
        self.register_buffer("offsets_list", torch.tensor(offsets, dtype=torch.int32))
        self.register_buffer("resolutions_list", torch.tensor([int(r) for r in resolutions], dtype=torch.int32))
        self.params = nn.Parameter(torch.empty(offsets[-1], n_features))
        self.reset_parameters()

    def reset_parameters(self):
        self.params.data.uniform_(-1e-4, 1e-4)

    def forward(self, inputs, min_level=0, n_levels=None):
        prefix = list(inputs.shape[:-1])
        n = self.n_levels - min_level if n_levels is None else n_levels
        out = grid_encode(inputs.reshape(-1, self.num_dim), self.params, self.offsets_list, self.resolutions_list,
                          min_level, n)
        return out.view(prefix + [n * self.n_features])
