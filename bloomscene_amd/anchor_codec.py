"""The anchor position coder on the MI355X, in HIP behind ``include/bloomscene_anchor_codec.h``: the one stream of a
compressed scene that BloomScene's ``GaussianModel.conduct_encoding`` never writes (it pickles ``_anchor``, 96 bits an
anchor, ``scene/gaussian_model.py:1112``, and reports 48).  The 16-bit lattice indices of ``Quantize_anchor`` are packed
into 48-bit keys, sorted, and their gaps coded with a per-chunk Golomb-Rice rule; the decoder returns ``get_anchor``'s
values bit for bit.

    stream, perm = encode_anchors(pc._anchor, pc.x_bound_min, pc.x_bound_max, rows=None)   # uint8 on the device, int64 [n]
    anchor, bound_min, bound_max = decode_anchors(stream)                                   # [n, 3], [3], [3]
    keys = lattice_keys(pc._anchor, pc.x_bound_min, pc.x_bound_max, rows=None)              # int64 [n], for measurement

The stream codes the rows in ascending key (ties in ascending source row, whatever the order of a row list): ``perm`` says which source row
each coded row is, and the caller applies it to every per-anchor tensor before coding the attributes.  ``rows`` is an int64
list or a bool mask ``[N]`` of the anchors to keep (the ``mask_anchor`` filter of ``scene/gaussian_model.py:1081-1083``).
The sort is torch's stable sort of the keys; everything else is this package's kernels.  Everything runs on the current
torch stream and takes the stream's bound and the scratch from torch's allocator; a call ends in ONE host read, of the
status word and the length, and raises ``ValueError`` naming the offence.  Two things cost a second read and say so: a
bool mask for ``rows`` (``torch.nonzero`` has to size its result) and ``decode_anchors`` of a stream that is on the
device without ``n=`` (the header's ``n`` sizes the output; a stream on the CPU, as read from a file, is parsed there).
Results are bit-identical from run to run.  There is no CPU path; importing this module needs no GPU.
"""
from __future__ import annotations

import struct

import torch

from . import _capi
from . import _operands as _ops
from ._operands import ptr

MAGIC, FORMAT, HEADER_BYTES, CHUNK, ESCAPE = 0x41525342, 1, 48, 256, 32   # BSR_ANCHOR_CODEC_*
MAX_N = 1 << 27                                                           # BSR_ANCHOR_CODEC_MAX_N
STATUS = (                                                                # BSR_ANCHOR_CODEC_* in bit order
    "a non-finite coordinate (or bounds that give no finite lattice index)",
    "a row outside [0, N)",
    "keys that are not ascending",
    "a key of 2^48 or more",
    "not a stream of this coder for this n (magic, format, chunk size, escape length, n, chunk count or bounds)",
    "a truncated stream",
    "a corrupt stream",
)


def _raise_status(who, status):
    if status:
        raise ValueError(f"{who}: " + "; ".join(text for bit, text in enumerate(STATUS) if status >> bit & 1))


def _source(who, _anchor, bound_min, bound_max, rows):
    """The checked operands of the lattice pass, in ``_operands``' order of complaints -> (anchor as the kernel reads it, N,
    its row stride, bound_min [3], bound_max [3], the row list or None, n)."""
    named = [("_anchor", _anchor), ("bound_min", bound_min), ("bound_max", bound_max)]
    _ops.check_tensors(who, named)
    if rows is not None:
        _ops.check_tensors(who, [("rows", rows)], (torch.int64, torch.bool), half_note=False)
        named.append(("rows", rows))
    if _anchor.dim() != 2:
        raise NotImplementedError(f"{who}: an _anchor of {_anchor.dim()} dimensions is not supported ([N, 3])")
    if _anchor.shape[1] != 3:
        raise ValueError(f"{who}: _anchor must be [N, 3] (got {list(_anchor.shape)})")
    N = _anchor.shape[0]
    for name, t in named[1:3]:
        if t.numel() != 3:
            raise ValueError(f"{who}: {name} must hold 3 values (got {list(t.shape)})")
    if rows is not None:
        if rows.dim() != 1 or (rows.dtype == torch.bool and rows.shape[0] != N):
            raise ValueError(f"{who}: rows must be an int64 list [n] or a bool mask [{N}] (got {rows.dtype} {list(rows.shape)})")
    if N > MAX_N:
        raise ValueError(f"{who}: at most 2^27 anchors (_anchor has {N})")
    if rows is not None and rows.shape[0] > MAX_N:
        raise ValueError(f"{who}: at most 2^27 rows (rows has {rows.shape[0]})")
    _ops.check_on_gpu(who, named)
    _ops.check_same_device(who, named, _anchor.device)
    if rows is not None:
        rows = (torch.nonzero(rows).reshape(-1) if rows.dtype == torch.bool else rows.detach()).contiguous()
    anchor = _ops.rows_in_place(_anchor.detach(), N, 3)
    n = N if rows is None else rows.shape[0]
    return (anchor, N, _ops.row_stride(anchor, N, 3), bound_min.detach().reshape(3).contiguous(),
            bound_max.detach().reshape(3).contiguous(), rows, n)


def _keys(anchor, N, stride, bmin, bmax, rows, n):
    """-> (keys int64 [n] in the row list's order, the two result words on the device)."""
    dev = anchor.device
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    result = torch.empty(2, dtype=torch.int32, device=dev)
    _capi.call("bsr_anchor_keys", N, n, ptr(anchor), stride, ptr(bmin), ptr(bmax), ptr(rows), ptr(keys), ptr(result),
               _ops.stream(dev))
    return keys, result


@torch.no_grad()
def lattice_keys(_anchor, bound_min, bound_max, rows=None):
    """The 48-bit keys ``x << 32 | y << 16 | z`` of the rows, int64 ``[n]`` in the row list's order (unsorted)."""
    who = "lattice_keys"
    keys, result = _keys(*_source(who, _anchor, bound_min, bound_max, rows))
    _raise_status(who, result.tolist()[0] & 0xffffffff)   # the call's one host read
    return keys


@torch.no_grad()
def encode_anchors(_anchor, bound_min, bound_max, rows=None):
    """``_anchor`` float32 ``[N, 3]`` (read in place through its row stride), the bounds ``[3]`` / ``[1, 3]`` as
    ``update_anchor_bound`` leaves them, ``rows`` None, an int64 list ``[n]`` or a bool mask ``[N]``.
    -> ``(stream, perm)``: the stream, a uint8 device tensor (a view of a bound-sized allocation, sliced to its length), and
    the int64 ``[n]`` source row of each coded row.  Raises ``ValueError`` for a non-finite coordinate or bound and for a
    row outside ``[0, N)``."""
    who = "encode_anchors"
    anchor, N, stride, bmin, bmax, rows, n = _source(who, _anchor, bound_min, bound_max, rows)
    dev = anchor.device
    keys, result = _keys(anchor, N, stride, bmin, bmax, rows, n)
    if rows is not None:                                 # ties go by SOURCE row: a list is put in ascending order first
        rows, by_row = torch.sort(rows, stable=True)     # (a no-op permutation for a mask's list, which ascends)
        keys = keys[by_row]
    keys, order = torch.sort(keys, stable=True)          # (keys are below 2^48: int64 order is theirs)
    perm = order if rows is None else rows[order]
    lib = _capi.lib()
    stream = torch.empty(lib.bsr_anchor_codec_stream_bound(n), dtype=torch.uint8, device=dev)
    scratch = _ops.scratch(lib.bsr_anchor_codec_scratch_bytes(n), dev)
    _capi.call("bsr_anchor_codec_encode", n, ptr(keys), ptr(bmin), ptr(bmax), ptr(stream), stream.numel(), ptr(result),
               ptr(scratch), _ops.stream(dev))
    status, length = result.tolist()                     # the call's one host read (the keys' status is in it)
    _raise_status(who, status & 0xffffffff)
    return stream[:length], perm


def _header_n(who, stream):
    """n of a stream's header, read where the stream is."""
    if stream.numel() < HEADER_BYTES:
        raise ValueError(f"{who}: {STATUS[5]}")
    magic, fmt, n = struct.unpack("<3I", bytes(stream[:12].tolist()))
    if magic != MAGIC or fmt != FORMAT or n > MAX_N:
        raise ValueError(f"{who}: {STATUS[4]}")
    return n


@torch.no_grad()
def decode_anchors(stream, n=None, device=None, return_keys=False):
    """The inverse: ``stream`` uint8 ``[bytes]`` -> ``(anchor [n, 3] float32, bound_min [3], bound_max [3])`` on the
    device, the anchors ``get_anchor``'s values bit for bit, in key order; with ``return_keys`` also the int64 keys.
    A stream on the CPU is parsed for ``n`` there and uploaded to ``device`` (a GPU; default: the current one; ``device`` is
    not looked at for a stream that is on a GPU already).  Raises
    ``ValueError`` for a stream that is not one of this coder, is truncated or is corrupt; the kernels never read beyond
    ``stream``'s own bytes."""
    who = "decode_anchors"
    _ops.check_tensors(who, [("stream", stream)], torch.uint8)
    if stream.dim() != 1:
        raise ValueError(f"{who}: stream must have one dimension (got {list(stream.shape)})")
    if n is not None and not 0 <= int(n) <= MAX_N:
        raise ValueError(f"{who}: n must be in [0, 2^27] (got {n})")
    if stream.device.type != "cuda" and device is not None and torch.device(device).type != "cuda":
        raise ValueError(f"{who}: device must be a GPU (there is no CPU path; got {device})")
    n = _header_n(who, stream) if n is None else int(n)
    if stream.device.type != "cuda":
        stream = stream.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    dev = stream.device
    if stream.stride(0) != 1 or stream.data_ptr() % 4:   # the kernels read 32-bit words
        stream = stream.clone(memory_format=torch.contiguous_format)
    anchor = torch.empty(n, 3, dtype=torch.float32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev) if return_keys else None
    bounds = torch.empty(6, dtype=torch.float32, device=dev)
    result = torch.empty(2, dtype=torch.int32, device=dev)
    _capi.call("bsr_anchor_codec_decode", n, ptr(stream), stream.numel(), ptr(anchor), ptr(keys), ptr(bounds), ptr(result),
               _ops.stream(dev))
    _raise_status(who, result.tolist()[0] & 0xffffffff)  # the call's one host read
    out = (anchor, bounds[:3], bounds[3:])
    return out + (keys,) if return_keys else out
