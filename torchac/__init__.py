"""Import shim: BloomScene's ``utils/encodings.py:6`` does ``import torchac`` (the arithmetic-coding extension) and calls
two of its functions, ``encode_float_cdf`` and ``decode_float_cdf``.  With this repository on ``sys.path`` that import
resolves here, to the table model of the MI355X-native rANS coder of ``bloomscene_amd.codec`` (C ABI
``include/bloomscene_codec.h``).  Importing needs no GPU.

``encode_float_cdf(cdf_float, sym, needs_normalization=True, check_input_bounds=False) -> bytes`` and
``decode_float_cdf(cdf_float, byte_stream, needs_normalization=True) -> int16 tensor`` with the extension's signatures:
``cdf_float`` float32 ``[..., L + 1]``, every row non-decreasing from 0 to 1, ``sym`` int16 ``[...]`` in ``[0, L)``.  CPU
tensors (the reference hands over ``.cpu()`` copies) are uploaded to the current device; the decoded symbols come back on
``cdf_float``'s device.  A row outside ``[0, 1]`` or not non-decreasing, or a symbol outside ``[0, L)``, always raises
``ValueError`` (``check_input_bounds`` is accepted and not needed).

THE BYTES ARE NOT torchac's: the format is this repository's own (``include/bloomscene_codec.h``), so a stream written
here is read here and nowhere else.  Every other name of the package raises NotImplementedError.
"""
import torch

from bloomscene_amd import codec as _codec


def _device(t):
    return t.device if t.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())


def _rows(who, cdf_float):
    if not isinstance(cdf_float, torch.Tensor):
        raise TypeError(f"{who}: cdf_float must be a torch.Tensor (got {type(cdf_float).__name__})")
    if cdf_float.dtype != torch.float32:
        raise TypeError(f"{who}: cdf_float must be float32 (got {cdf_float.dtype})")
    if cdf_float.dim() < 2:
        raise ValueError(f"{who}: cdf_float must be [..., L + 1] with at least two dimensions (got {list(cdf_float.shape)})")
    return cdf_float.reshape(-1, cdf_float.shape[-1])


def encode_float_cdf(cdf_float, sym, needs_normalization=True, check_input_bounds=False):
    who = "torchac.encode_float_cdf"
    rows = _rows(who, cdf_float)
    if not isinstance(sym, torch.Tensor):
        raise TypeError(f"{who}: sym must be a torch.Tensor (got {type(sym).__name__})")
    if sym.dtype != torch.int16:
        raise TypeError(f"{who}: sym must be int16 (got {sym.dtype})")
    if tuple(sym.shape) != tuple(cdf_float.shape[:-1]):
        raise ValueError(f"{who}: sym must be {list(cdf_float.shape[:-1])} (got {list(sym.shape)})")
    dev = _device(cdf_float)
    stream = _codec.encode_symbols(sym.reshape(-1).to(dev), rows.to(dev))
    return stream.cpu().numpy().tobytes()


def decode_float_cdf(cdf_float, byte_stream, needs_normalization=True):
    who = "torchac.decode_float_cdf"
    rows = _rows(who, cdf_float)
    if not isinstance(byte_stream, (bytes, bytearray)):
        raise TypeError(f"{who}: byte_stream must be bytes (got {type(byte_stream).__name__})")
    dev = _device(cdf_float)
    stream = (torch.frombuffer(bytearray(byte_stream), dtype=torch.uint8) if len(byte_stream)
              else torch.empty(0, dtype=torch.uint8)).to(dev)
    sym = _codec.decode_symbols(stream, rows.to(dev), rows.shape[0])
    return sym.reshape(cdf_float.shape[:-1]).to(cdf_float.device)


def _unsupported(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"torchac.{name} is not implemented on this backend (BloomScene does not call it)")
    fn.__name__ = name
    return fn


encode_int16_normalized_cdf = _unsupported("encode_int16_normalized_cdf")
decode_int16_normalized_cdf = _unsupported("decode_int16_normalized_cdf")
encode_cdf = _unsupported("encode_cdf")
decode_cdf = _unsupported("decode_cdf")


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return _unsupported(name)
