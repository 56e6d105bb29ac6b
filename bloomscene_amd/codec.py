"""The entropy codec on the MI355X: what BloomScene's ``utils/encodings.py:84-174`` ("UE") does through torchac -- a table
of Gaussian cdf values built on the GPU per batch of 1 000 anchors, copied to the host and fed to a sequential CPU
arithmetic coder -- as an interleaved rANS coder in HIP behind ``include/bloomscene_codec.h``.  No table is built: a lane
evaluates the two integer cdf values of its own symbol from ``(mean, scale, Q)``, and the decoder runs the same device
function, so its model is the encoder's bit for bit.

    stream = encode_gaussian(x, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9)     # uint8, on the device
    y = decode_gaussian(stream, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9)     # rint(x / Q) * Q, [n, C]
    stream = encode_symbols(sym, cdf);  sym = decode_symbols(stream, cdf, n)                  # a caller's cdf table
    bit_len, lo, hi = encoder_gaussian(x, mean, scale, Q, file_name);  decoder_gaussian(...)  # UE's four, one file each
    bit_len = encoder(x, p, file_name);  x = decoder(p, file_name)
    streams = encode_attributes(context, Q, feat_q, scaling_q, offsets_q, masks, F, K)         # the whole model at once
    feat_q, scaling_q, offsets_q = decode_attributes(streams, context, Q, masks, F, K)

THE FORMAT IS OUR OWN (header, offset table, per chunk of ``64 T`` symbols 64 final states and the 16-bit words): it is
not byte-compatible with torchac's and a stream written here is read here.  The function, the integer model and the
layout are written out in the header.  ``x``, ``mean``, ``scale`` are read in place through their row stride (``mean`` and
``scale`` as column blocks of the ``[n, O]`` context cost no copy).  Everything runs on the current torch stream and takes
the stream's bound and the scratch from torch's allocator; every call ends in ONE host read, of the status word and the
length, and raises ``ValueError`` naming the offence.  There is no CPU path; importing this module needs no GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from . import _operands as _ops
from ._operands import ptr, row_stride

Q_SINGLE, Q_ROW, Q_ELEMENT = 0, 1, 2          # BSR_CODEC_Q_*
DEFAULT_STEPS = 256                           # BSR_CODEC_DEFAULT_STEPS
MAX_SYMBOLS = 32767                           # BSR_CODEC_MAX_SYMBOLS
MAX_ELEMENTS = 1 << 30                        # BSR_CODEC_MAX_ELEMENTS
HEADER_BYTES = 32
STATUS = (                                    # BSR_CODEC_BAD_* in bit order
    "a non-finite x / Q, or |rint(x / Q)| of 2^30 or more",
    "Q <= 0 or not finite",
    "a non-finite mean or scale",
    f"more than {MAX_SYMBOLS} symbols between the smallest and the largest rint(x / Q)",
    "a cdf row that is not non-decreasing within [0, 1]",
    "a symbol outside [0, L)",
    "not a stream of this codec for these operands (magic, version, model kind, element count, L or T)",
    "a truncated stream",
    "a corrupt stream",
)


def _raise_status(who, status):
    if status:
        raise ValueError(f"{who}: " + "; ".join(text for bit, text in enumerate(STATUS) if status >> bit & 1))


class _Gaussian:
    """The checked operands of one Gaussian call, in ``_operands``' order of complaints (``keep`` may also be bool)."""

    def __init__(self, who, x, mean, scale, Q, keep, keep_repeat, scale_min, stream=None):
        named = ([("x", x)] if stream is None else []) + [("mean", mean), ("scale", scale)]
        if isinstance(Q, torch.Tensor):
            named.append(("Q", Q))
        elif not isinstance(Q, (int, float)):
            raise TypeError(f"{who}: Q must be a number or a torch.Tensor (got {type(Q).__name__})")
        _ops.check_tensors(who, named)
        if keep is not None:
            if not (isinstance(keep, torch.Tensor) and keep.dtype == torch.bool):   # (a bool mask is taken as it is)
                _ops.check_tensors(who, [("keep", keep)])
            named.append(("keep", keep))
        if stream is not None:
            _check_stream(who, stream)
        lead = mean if stream is not None else x
        if lead.dim() not in (1, 2):
            raise NotImplementedError(f"{who}: operands of {lead.dim()} dimensions are not supported (one or two)")
        shape = tuple(lead.shape)
        flat = lead.dim() == 1
        n, C = (shape[0], 1) if flat else shape
        if C < 1:
            raise ValueError(f"{who}: need at least one column (got {list(shape)})")
        for name, t in named[:3 if stream is None else 2]:
            if tuple(t.shape) != shape:
                raise ValueError(f"{who}: {name} must be {list(shape)} (got {list(t.shape)})")
        r = int(keep_repeat)
        if r < 1 or C % r != 0:
            raise ValueError(f"{who}: keep_repeat must divide C = {C} (got {keep_repeat})")
        if keep is None and r != 1:
            raise ValueError(f"{who}: keep_repeat = {r} without keep")
        if n * C > MAX_ELEMENTS:
            raise ValueError(f"{who}: at most 2^30 elements (got {n} * {C})")
        if not (float(scale_min) > 0.0 and float(scale_min) < float("inf")):
            raise ValueError(f"{who}: scale_min must be positive and finite (got {scale_min})")
        dev = lead.device
        if isinstance(Q, torch.Tensor):
            if Q.numel() == 1:
                self.q_mode, q = Q_SINGLE, Q.reshape(1)
            elif tuple(Q.shape) in ((n, 1), (n,)):
                self.q_mode, q = Q_ROW, Q.reshape(n)
            elif tuple(Q.shape) == (n, C):
                self.q_mode, q = Q_ELEMENT, Q
            else:
                raise ValueError(f"{who}: Q must be a scalar, [{n}, 1] or [{n}, {C}] (got {list(Q.shape)})")
            q = q.detach().contiguous()
        else:
            self.q_mode, q = Q_SINGLE, None
        if keep is not None:
            if keep.numel() != n * (C // r) or (keep.dim() > 0 and keep.shape[0] != n and n > 0):
                raise ValueError(f"{who}: keep must be [{n}, {C // r}] (got {list(keep.shape)})")
        placed = named + ([("stream", stream)] if stream is not None else [])
        _ops.check_on_gpu(who, placed)
        _ops.check_same_device(who, placed, dev)
        if q is None:
            q = torch.full((1,), float(Q), dtype=torch.float32, device=dev)
        if keep is not None:
            keep = keep.detach().reshape(n, C // r).to(torch.float32).contiguous()
        self.n, self.C, self.r, self.q, self.keep, self.shape, self.dev = n, C, r, q, keep, shape, dev
        self.scale_min = float(scale_min)
        two = lambda t: _ops.rows_in_place(t.detach().reshape(n, C), n, C)
        self.x = None if stream is not None else two(x)
        self.mean, self.scale = two(mean), two(scale)


def _check_stream(who, stream):
    _ops.check_tensors(who, [("stream", stream)], torch.uint8)
    if stream.dim() != 1:
        raise ValueError(f"{who}: stream must have one dimension (got {list(stream.shape)})")


def _aligned(stream):
    """The kernels read the stream as 32-bit words: a view that starts elsewhere (or is strided) is copied."""
    if stream.stride(0) != 1 or stream.data_ptr() % 4:
        return stream.clone(memory_format=torch.contiguous_format)
    return stream


def _steps(who, T):
    T = int(T)
    if not 1 <= T <= 65536:
        raise ValueError(f"{who}: T must be in [1, 65536] (got {T})")
    return T


def _buffers(who, elements, T, dev):
    lib = _capi.lib()
    bound = lib.bsr_codec_stream_bound(elements, T)
    if bound == 0:
        raise ValueError(f"{who}: {elements} elements with T = {T} are not supported (the stream could pass 2^32 bytes)")
    stream = torch.empty(bound, dtype=torch.uint8, device=dev)
    scratch = _ops.scratch(lib.bsr_codec_scratch_bytes(elements, T), dev)
    result = torch.empty(2, dtype=torch.int32, device=dev)
    return stream, scratch, result


def _finish_encode(who, stream, result):
    status, length = result.tolist()          # the call's one host read
    _raise_status(who, status & 0xffffffff)
    return stream[:length]


@torch.no_grad()
def encode_gaussian(x, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9, T=DEFAULT_STEPS):
    """``x``, ``mean``, ``scale`` float32 ``[n, C]`` (or ``[n]``) on the GPU; ``Q`` a number or a tensor (one value,
    ``[n]`` / ``[n, 1]`` or ``[n, C]``); ``keep`` ``[n, C / keep_repeat]`` (float or bool): an element whose entry is 0 is
    skipped and decodes as 0.  -> the stream, a uint8 device tensor: a view of a bound-sized allocation, sliced to its
    length.  Raises ``ValueError`` for a non-finite ``x / Q``, ``Q <= 0``, a non-finite ``mean`` or ``scale``, or a span of
    more than 32 767 steps between the smallest and the largest ``rint(x / Q)``."""
    who = "encode_gaussian"
    op = _Gaussian(who, x, mean, scale, Q, keep, keep_repeat, scale_min)
    T = _steps(who, T)
    n, C = op.n, op.C
    stream, scratch, result = _buffers(who, n * C, T, op.dev)
    _capi.call("bsr_codec_encode_gaussian", n, C, op.r, ptr(op.x), row_stride(op.x, n, C), ptr(op.mean),
               row_stride(op.mean, n, C), ptr(op.scale), row_stride(op.scale, n, C), ptr(op.q), op.q_mode, ptr(op.keep),
               op.scale_min, T, ptr(stream), stream.numel(), ptr(result), ptr(scratch), _ops.stream(op.dev))
    return _finish_encode(who, stream, result)


@torch.no_grad()
def decode_gaussian(stream, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9):
    """The inverse: the operands of ``encode_gaussian`` without ``x`` -> float32 in ``mean``'s shape, ``rint(x / Q) * Q``
    bit for bit, 0 where skipped.  Raises ``ValueError`` for a stream that is not one of this codec for these operands,
    is truncated or is corrupt; the kernels never read beyond ``stream``'s own bytes."""
    who = "decode_gaussian"
    op = _Gaussian(who, None, mean, scale, Q, keep, keep_repeat, scale_min, stream=stream)
    n, C = op.n, op.C
    stream = _aligned(stream)
    out = torch.empty(n, C, dtype=torch.float32, device=op.dev)
    result = torch.empty(2, dtype=torch.int32, device=op.dev)
    _capi.call("bsr_codec_decode_gaussian", n, C, op.r, ptr(stream), stream.numel(), ptr(op.mean),
               row_stride(op.mean, n, C), ptr(op.scale), row_stride(op.scale, n, C), ptr(op.q), op.q_mode, ptr(op.keep),
               op.scale_min, ptr(out), ptr(result), _ops.stream(op.dev))
    _raise_status(who, result.tolist()[0] & 0xffffffff)
    return out.reshape(op.shape)


def _table(who, cdf, n):
    """-> (cdf as the kernel reads it, L, row stride)."""
    _ops.check_tensors(who, [("cdf", cdf)], half_note=False)
    if cdf.dim() not in (1, 2):
        raise NotImplementedError(f"{who}: a cdf of {cdf.dim()} dimensions is not supported ([L + 1] or [rows, L + 1])")
    L = cdf.shape[-1] - 1
    if not 1 <= L <= MAX_SYMBOLS:
        raise ValueError(f"{who}: cdf needs 2 to {MAX_SYMBOLS + 1} columns (got {cdf.shape[-1]})")
    if cdf.dim() == 2 and cdf.shape[0] != n:
        raise ValueError(f"{who}: cdf must have one row per symbol, {n} (got {cdf.shape[0]}), or be one row [L + 1]")
    if n > MAX_ELEMENTS:
        raise ValueError(f"{who}: at most 2^30 symbols (got {n})")
    return L, (0 if cdf.dim() == 1 else L + 1)


@torch.no_grad()
def encode_symbols(sym, cdf, T=DEFAULT_STEPS):
    """The table model: ``sym`` int16 ``[n]`` in ``[0, L)``, ``cdf`` float32 ``[L + 1]`` (one row for every symbol) or
    ``[n, L + 1]``, each row non-decreasing from 0 to 1.  -> the stream."""
    who = "encode_symbols"
    _ops.check_tensors(who, [("sym", sym)], torch.int16)
    n = sym.numel()
    L, cs = _table(who, cdf, n)
    T = _steps(who, T)
    _ops.check_on_gpu(who, [("sym", sym), ("cdf", cdf)])
    _ops.check_same_device(who, [("cdf", cdf)], sym.device)
    sym, cdf = sym.reshape(n).contiguous(), cdf.detach().contiguous()
    stream, scratch, result = _buffers(who, n, T, sym.device)
    _capi.call("bsr_codec_encode_table", n, L, ptr(sym), ptr(cdf), cs, T, ptr(stream), stream.numel(), ptr(result),
               ptr(scratch), _ops.stream(sym.device))
    return _finish_encode(who, stream, result)


@torch.no_grad()
def decode_symbols(stream, cdf, n):
    """-> int16 ``[n]``, the symbols ``encode_symbols`` was given, from the same ``cdf``."""
    who = "decode_symbols"
    n = int(n)
    _ops.check_tensors(who, [("cdf", cdf)], None)
    _check_stream(who, stream)
    if n < 0:
        raise ValueError(f"{who}: n must not be negative (got {n})")
    L, cs = _table(who, cdf, n)
    _ops.check_on_gpu(who, [("stream", stream), ("cdf", cdf)])
    _ops.check_same_device(who, [("cdf", cdf)], stream.device)
    stream, cdf = _aligned(stream), cdf.detach().contiguous()
    out = torch.empty(n, dtype=torch.int16, device=stream.device)
    result = torch.empty(2, dtype=torch.int32, device=stream.device)
    _capi.call("bsr_codec_decode_table", n, L, ptr(stream), stream.numel(), ptr(cdf), cs, ptr(out), ptr(result),
               _ops.stream(stream.device))
    _raise_status(who, result.tolist()[0] & 0xffffffff)
    return out


# ---- the drop-ins of utils/encodings.py: same signatures, ONE file each (the use_multiprocessor split is gone) ----
def _write(stream, file_name):
    assert file_name.endswith(".b")
    host = stream.cpu().numpy()
    with open(file_name, "wb") as f:
        f.write(host.tobytes())
    return host


def _read(file_name, device):
    assert file_name.endswith(".b")
    with open(file_name, "rb") as f:
        data = f.read()
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if data else torch.empty(0, dtype=torch.uint8, device=device)


def encoder_gaussian(x, mean, scale, Q, file_name="tmp.b"):
    """UE:84-114 -> ``(bit_len, min_value, max_value)``: the file's bits and the smallest and largest ``rint(x / Q)`` as
    0-dim tensors (the stream's header carries them: ``decoder_gaussian`` does not need them back)."""
    host = _write(encode_gaussian(x, mean, scale, Q), file_name)
    header = host[:HEADER_BYTES].view(np.int32)
    lo, L = int(header[4]), int(header[5])
    return host.size * 8, torch.tensor(float(lo), device=x.device), torch.tensor(float(lo + max(L, 1) - 1), device=x.device)


def decoder_gaussian(mean, scale, Q, file_name="tmp.b", min_value=-100, max_value=100):
    """UE:117-138.  ``min_value`` / ``max_value`` are accepted and not read: the header has them."""
    return decode_gaussian(_read(file_name, mean.device), mean, scale, Q)


def bernoulli_cdf(p):
    """The cdf table of a Bernoulli coder, ``[0, 1 - p, 1]`` per element of ``p`` (UE:145-149), or one row ``[3]`` for a
    single ``p``: what ``encode_symbols`` / ``decode_symbols`` take for symbols 0 / 1 with ``p`` the probability of 1.
    ``p = 0`` or ``1`` is legal: the symbol without mass keeps the model's floor of two counts."""
    p = p.detach().to(torch.float32).reshape(-1)
    pu = 1 - p.unsqueeze(-1)
    cdf = torch.cat([torch.zeros_like(pu), pu, torch.ones_like(pu)], dim=-1)
    return cdf[0] if p.numel() == 1 else cdf


def encoder(x, p, file_name):
    """UE:141-157: ``x`` in {-1, +1}, ``p`` the probability of +1 (per element, or one value) -> the file's bits."""
    dev = x.device if x.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    sym = torch.floor((x.detach().to(dev).reshape(-1) + 1) / 2).to(torch.int16)
    return _write(encode_symbols(sym, bernoulli_cdf(p.to(dev))), file_name).size * 8


def decoder(p, file_name):
    """UE:159-174 -> {-1, +1} float32 on ``p``'s device."""
    dev = p.device if p.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    n = p.numel()
    sym = decode_symbols(_read(file_name, dev), bernoulli_cdf(p.to(dev)), n)
    return (sym * 2 - 1).to(torch.float32).to(p.device)


# ---- the whole model at once ----
def _blocks(who, context, Q, F, K):
    F, K = int(F), int(K)
    if not isinstance(context, torch.Tensor) or not isinstance(Q, torch.Tensor):
        raise TypeError(f"{who}: context and Q must be tensors")
    O = 2 * F + 12 + 6 * K + 3
    if context.dim() != 2 or context.shape[1] != O:
        raise ValueError(f"{who}: context must be [n, {O}] (got {list(context.shape)})")
    n = context.shape[0]
    if tuple(Q.shape) != (n, 3):
        raise ValueError(f"{who}: Q must be [{n}, 3] (got {list(Q.shape)})")
    mean, scale, mean_s, scale_s, mean_o, scale_o, _ = torch.split(context, [F, F, 6, 6, 3 * K, 3 * K, 3], dim=-1)
    return n, ((mean, scale, Q[:, 0]), (mean_s, scale_s, Q[:, 1]), (mean_o, scale_o, Q[:, 2]))


def encode_attributes(context, Q, feat_q, scaling_q, offsets_q, masks, F, K, T=DEFAULT_STEPS):
    """The three streams of the anchors' attributes, all anchors at once (no batches of 1 000: there is no table).
    ``context [n, 2 F + 12 + 6 K + 3]`` and ``Q [n, 3]`` as ``context.context_head_maps`` /
    ``context_quantise(..., steps=True)`` return them (the means and scales are column blocks, read in place);
    ``feat_q [n, F]``, ``scaling_q [n, 6]``, ``offsets_q [n, K, 3]`` the quantised attributes; ``masks [n, K, 1]`` (or
    ``[n, K]``): the offsets of a masked-out Gaussian are skipped.  -> ``(feat, scaling, offsets)`` streams."""
    who = "encode_attributes"
    n, blocks = _blocks(who, context, Q, F, K)
    xs = (feat_q, scaling_q, offsets_q.reshape(n, 3 * int(K)))
    keeps = (None, None, masks.reshape(n, int(K)))
    return tuple(encode_gaussian(x, m, s, q, keep=k, keep_repeat=3 if k is not None else 1, T=T)
                 for x, (m, s, q), k in zip(xs, blocks, keeps))


def decode_attributes(streams, context, Q, masks, F, K):
    """The inverse -> ``(feat_q [n, F], scaling_q [n, 6], offsets_q [n, K, 3])``, each ``rint(x / Q) * Q``; the offsets
    of a masked-out Gaussian are 0."""
    who = "decode_attributes"
    n, blocks = _blocks(who, context, Q, F, K)
    if len(streams) != 3:
        raise ValueError(f"{who}: three streams (feat, scaling, offsets) are needed (got {len(streams)})")
    keeps = (None, None, masks.reshape(n, int(K)))
    feat, scaling, offsets = (decode_gaussian(st, m, s, q, keep=k, keep_repeat=3 if k is not None else 1)
                              for st, (m, s, q), k in zip(streams, blocks, keeps))
    return feat, scaling, offsets.reshape(n, int(K), 3)
