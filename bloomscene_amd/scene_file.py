"""A compressed BloomScene scene as ONE self-contained file: what ``GaussianModel.conduct_encoding`` /
``conduct_decoding`` (``scene/gaussian_model.py:1075-1368``, "GM") spread over ``anchor.pkl``, ``hash.b``, ``masks.b``, three
``.b`` files per 1 000 anchors and a Python list handed over in memory -- plus a live model for the MLPs and the table
shapes.  ``load_scene`` takes the path and nothing else.

    info = save_scene(path, anchor=pc._anchor, bound_min=pc.x_bound_min, bound_max=pc.x_bound_max,
                      anchor_feat=pc._anchor_feat, offset=pc._offset, scaling=pc.get_scaling, mask=pc.get_mask,
                      encoding=pc.encoding_xyz, mlp_grid=pc.mlp_grid, mlps={"mlp_opacity": ..., "mlp_cov": ..., "mlp_color": ...},
                      F=pc.feat_dim, K=pc.n_offsets)                      # -> SceneInfo(perm, keep, bytes per section)
    info = save_model(pc, path)                                           # the same, read off a reference GaussianModel
    scene = load_scene(path, device);  scene.apply_to(pc)                 # GM:1344-1368

THE FILE, little endian: ``"BSRS"``, format 1; ``n, F, K``; the ``MixEncoding`` constructor arguments (``n_features``, the
two ``log2_hashmap_size``, the two resolution lists); per MLP its name, its three layer widths and what follows its second
``Linear`` (nothing, ``Tanh``, ``Sigmoid``); the section table (kind, offset, length, each section 8-byte aligned); then the
sections IN DECODE ORDER:

  1. the MLP parameters, raw fp32, W1 b1 W2 b2 of each MLP in the header's order (what ``get_mlp_size`` counts)
  2. the hash tables' signs, per table: fp32 p, uint32 count, then ``codec.encode_symbols`` of the signs under Bernoulli(p)
     (GM:1192-1197)
  3. the anchors: ``anchor_codec.encode_anchors`` (include/bloomscene_anchor_codec.h)
  4. the masks: fp32 p, uint32 count, then Bernoulli(p) over ``[n, K]`` (GM:1204-1208)
  5. - 7. the three attribute streams of ``codec.encode_attributes``; their ``context`` and ``Q`` come from ``encoding`` ->
     ``context.context_head_maps`` run on the DEQUANTISED, PERMUTED anchors and the tables' signs -- the decoder runs the
     same two calls on the decoded anchors and the decoded tables, so its model is the encoder's bit for bit.  The
     attributes are put on their steps by ``context.context_quantise_tensors(..., steps=True)``, whose ``Q`` the saver
     requires to be the head's bit for bit (it raises otherwise: the decoder has only the head's).

DEVIATIONS from GM.  Pruned anchors (every mask entry 0) are not written and not restored: GM pads them back as all-zero
rows, which render nothing.  Rows come back in key order (``SceneInfo.perm``).  The tables must be binary (``ste_binary``).
The saver reads the device a few times (the two probabilities, the streams' lengths); nothing here is on a training path.
"""
from __future__ import annotations

import struct
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _operands as _ops
from . import anchor_codec, codec, context
from .grid_encoder import SUPPORTED_FEATURES, table_offsets
from .mix_encoding import MAX_LEVELS, MixEncoding

MAGIC, FORMAT = b"BSRS", 1
SECTION_MLPS, SECTION_TABLE, SECTION_ANCHORS, SECTION_MASKS, SECTION_FEAT, SECTION_SCALING, SECTION_OFFSETS = range(1, 8)
SECTION_NAMES = {SECTION_MLPS: "mlps", SECTION_TABLE: "table", SECTION_ANCHORS: "anchors", SECTION_MASKS: "masks",
                 SECTION_FEAT: "feat", SECTION_SCALING: "scaling", SECTION_OFFSETS: "offsets"}
LAST_LAYERS = (None, nn.Tanh, nn.Sigmoid)        # the code of what follows an MLP's second Linear
GRID_MLP = "mlp_grid"
# what load_scene accepts of a header before it allocates from it
MAX_LOG2_ROWS, MAX_RESOLUTION, MAX_WIDTH = 24, 1 << 20, 4096
MAX_SYMBOLS_PER_BYTE = 64     # a Bernoulli stream holds 64 final states of 4 bytes per 16 384 symbols, whatever p is


class SceneInfo(SimpleNamespace):
    """What ``save_scene`` returns: ``perm`` (int64 ``[n]``: the source row of each written row), ``keep`` (bool ``[N]``),
    ``n``, ``sections`` (name -> bytes, padding included), ``header_bytes``, ``file_bytes`` (= header + sections)."""


def _mlp_weights(who, name, mlp):
    """-> (the code of the last layer, [W1, b1, W2, b2]); NotImplementedError for any other stack."""
    error = None
    for code, last in enumerate(LAST_LAYERS):
        try:
            return code, _ops.sequential_weights(who, name, mlp, last)
        except NotImplementedError as e:
            error = error or e
    raise error


def _bernoulli_section(x01):
    """[n] of 0 / 1 on the device -> the section's bytes: fp32 p = the share of ones, the count, the stream."""
    flat = x01.reshape(-1)
    p = np.float32(float(flat.sum()) / max(flat.numel(), 1))
    stream = codec.encode_symbols(flat.to(torch.int16), _bernoulli_cdf(p, flat.device))
    return struct.pack("<fI", p, flat.numel()) + stream.cpu().numpy().tobytes()


def _bernoulli_cdf(p, device):
    return codec.bernoulli_cdf(torch.tensor([float(p)], dtype=torch.float32, device=device))


def _bernoulli_decode(who, what, data, device, want):
    """A Bernoulli section -> int16 [want] of 0 / 1; the section's own count must be ``want`` (known from the header before
    anything is allocated)."""
    if len(data) < 8:
        raise ValueError(f"{who}: a truncated file ({what})")
    p, count = struct.unpack("<fI", data[:8])
    if count != want or not 0.0 <= p <= 1.0:
        raise ValueError(f"{who}: a corrupt file ({what}: {count} symbols with p = {p}, {want} are expected)")
    stream = torch.frombuffer(bytearray(data[8:]), dtype=torch.uint8).to(device)
    return codec.decode_symbols(stream, _bernoulli_cdf(np.float32(p), device), count)


def _model_operands(anchor_q, bound_min, bound_max, encoding, weights, F, K):
    """context [n, O] and Q [n, 3] of the coded anchors: the two calls both sides make."""
    enc = encoding(anchor_q, bound_min, bound_max)
    ctx, Q = context.context_head_maps(enc, weights, F, K)[:2]
    return enc, ctx, Q


@torch.no_grad()
def save_scene(path, *, anchor, bound_min, bound_max, anchor_feat, offset, scaling, mask, encoding, mlp_grid, mlps, F, K):
    """Plain tensors and modules -> the file.  ``anchor [N, 3]`` the raw ``_anchor``; the bounds ``[3]`` / ``[1, 3]``;
    ``anchor_feat [N, F]``; ``offset [N, K, 3]``; ``scaling [N, 6]`` as ``get_scaling`` returns it; ``mask [N, K, 1]`` or
    ``[N, K]`` of 0 / 1 as ``get_mask`` returns it; ``encoding`` a ``MixEncoding``; ``mlp_grid`` and the ``mlps`` (a mapping
    name -> module, kept in order) each ``Linear, ReLU, Linear [+ Tanh | Sigmoid]``.  -> ``SceneInfo``: ``perm`` (int64
    ``[n]``, the source row of each written row), ``keep`` (bool ``[N]``), ``sections`` (name -> bytes), ``header_bytes``,
    ``file_bytes``."""
    who = "save_scene"
    F, K = int(F), int(K)
    named = [("anchor", anchor), ("bound_min", bound_min), ("bound_max", bound_max), ("anchor_feat", anchor_feat),
             ("offset", offset), ("scaling", scaling), ("mask", mask)]
    _ops.check_tensors(who, named)
    if not isinstance(encoding, MixEncoding):
        raise NotImplementedError(f"{who}: encoding must be a MixEncoding (got {type(encoding).__name__})")
    if not encoding.ste_binary:
        raise NotImplementedError(f"{who}: only binary tables are written (ste_binary)")
    stacks = OrderedDict([(GRID_MLP, mlp_grid)] + [(str(k), m) for k, m in mlps.items()])
    coded = OrderedDict((name, _mlp_weights(who, name, m)) for name, m in stacks.items())
    if anchor.dim() != 2 or anchor.shape[1] != 3:
        raise ValueError(f"{who}: anchor must be [N, 3] (got {list(anchor.shape)})")
    N = anchor.shape[0]
    for name, t, shape in (("anchor_feat", anchor_feat, (N, F)), ("offset", offset, (N, K, 3)), ("scaling", scaling, (N, 6))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must be {list(shape)} (got {list(t.shape)})")
    if tuple(mask.shape) not in ((N, K, 1), (N, K)):
        raise ValueError(f"{who}: mask must be [{N}, {K}, 1] (got {list(mask.shape)})")
    for name, t in named[1:3]:
        if t.numel() != 3:
            raise ValueError(f"{who}: {name} must hold 3 values (got {list(t.shape)})")
    _ops.check_on_gpu(who, named)
    _ops.check_same_device(who, named, anchor.device)
    dev = anchor.device
    weights = [w.detach() for w in coded[GRID_MLP][1]]
    bmin, bmax = bound_min.detach().reshape(3), bound_max.detach().reshape(3)

    # the anchors first: everything else is coded in their order, under a model of their decoded values
    keep = (mask.detach().reshape(N, K) != 0).any(dim=1)
    anchor_stream, perm = anchor_codec.encode_anchors(anchor, bmin, bmax, rows=keep)
    n = perm.numel()
    anchor_q = anchor_codec.decode_anchors(anchor_stream, n=n)[0]
    mask_p = (mask.detach().reshape(N, K)[perm] != 0).to(torch.float32)
    sections = [(SECTION_MLPS, b"".join(w.detach().to(torch.float32).contiguous().cpu().numpy().tobytes()
                                        for _, ws in coded.values() for w in ws))]
    for e in (getattr(encoding, name) for name in MixEncoding.NAMES):
        sections.append((SECTION_TABLE, _bernoulli_section(e.params.detach() >= 0)))      # (+1 where p >= 0: STE_binary)
    sections.append((SECTION_ANCHORS, anchor_stream.cpu().numpy().tobytes()))
    sections.append((SECTION_MASKS, _bernoulli_section(mask_p)))
    if n > 0:
        signs = _signed_copy(encoding).to(dev)
        enc, ctx, Q = _model_operands(anchor_q, bmin, bmax, signs, weights, F, K)
        feat_p, scaling_p, offset_p = anchor_feat.detach()[perm], scaling.detach()[perm], offset.detach()[perm]
        feat_q, scaling_q, offsets_q, Q_steps = context.context_quantise_tensors(
            enc, weights, F, K, feat_p, scaling_p, offset_p, feat_p.mean(), scaling_p.mean(), offset_p.mean(), steps=True)
        if not torch.equal(Q_steps.view(torch.int32), Q.view(torch.int32)):    # (one more host read of the saver)
            raise RuntimeError(f"{who}: the quantiser's step sizes are not the context head's")
        streams = codec.encode_attributes(ctx, Q, feat_q, scaling_q, offsets_q * mask_p.unsqueeze(-1), mask_p, F, K)
    else:
        streams = [torch.empty(0, dtype=torch.uint8)] * 3
    for kind, s in zip((SECTION_FEAT, SECTION_SCALING, SECTION_OFFSETS), streams):
        sections.append((kind, s.cpu().numpy().tobytes()))

    head = bytearray(MAGIC + struct.pack("<4I", FORMAT, n, F, K))
    xyz, xy = encoding.encoding_xyz, encoding.encoding_xy
    lists = [[int(r) for r in e.resolutions_list.tolist()] for e in (xyz, xy)]
    head += struct.pack("<5I", xyz.n_features, xyz.log2_hashmap_size, xy.log2_hashmap_size, len(lists[0]), len(lists[1]))
    head += struct.pack(f"<{len(lists[0]) + len(lists[1])}I", *lists[0], *lists[1])
    head += struct.pack("<I", len(coded))
    for name, (code, ws) in coded.items():
        raw = name.encode("utf-8")
        head += struct.pack("<I", len(raw)) + raw + b"\0" * (-len(raw) % 4)
        head += struct.pack("<4I", ws[0].shape[1], ws[0].shape[0], ws[2].shape[0], code)
    head += struct.pack("<I", len(sections))
    at = len(head) + 20 * len(sections)
    at += -at % 8
    header_bytes, table, body = at, b"", bytearray()
    for kind, data in sections:
        table += struct.pack("<IQQ", kind, at, len(data))
        body += data + b"\0" * (-len(data) % 8)
        at += len(data) + (-len(data) % 8)
    head += table
    head += b"\0" * (header_bytes - len(head))
    with open(path, "wb") as f:
        f.write(head + body)
    sizes = OrderedDict()
    for kind, data in sections:
        key = SECTION_NAMES[kind]
        if kind == SECTION_TABLE:
            key = f"table_{sum(k.startswith('table') for k in sizes)}"
        sizes[key] = len(data) + (-len(data) % 8)
    return SceneInfo(perm=perm, keep=keep, n=n, sections=sizes, header_bytes=header_bytes, file_bytes=len(head) + len(body))


def _signed_copy(encoding):
    """A MixEncoding of the same shape whose tables hold the signs (+1 where p >= 0, else -1): what the decoder has."""
    xyz, xy = encoding.encoding_xyz, encoding.encoding_xy
    twin = MixEncoding(xyz.n_features, [int(r) for r in xyz.resolutions_list.tolist()], xyz.log2_hashmap_size,
                       [int(r) for r in xy.resolutions_list.tolist()], xy.log2_hashmap_size)
    for name in MixEncoding.NAMES:
        p = getattr(encoding, name).params.detach()
        getattr(twin, name).params.data = torch.where(p >= 0, 1.0, -1.0).to(torch.float32)
    return twin


def save_model(model, path):
    """``save_scene`` read off a reference ``GaussianModel`` (or anything with its attribute names): ``get_mask_anchor``,
    ``get_scaling`` and ``get_mask`` are applied as GM:1081-1087 do -- the anchors ``get_mask_anchor`` drops are exactly the
    ones with no mask entry set, which ``save_scene`` prunes."""
    return save_scene(path, anchor=model._anchor, bound_min=model.x_bound_min, bound_max=model.x_bound_max,
                      anchor_feat=model._anchor_feat, offset=model._offset, scaling=model.get_scaling, mask=model.get_mask,
                      encoding=model.encoding_xyz, mlp_grid=model.mlp_grid,
                      mlps=OrderedDict((k, getattr(model, k)) for k in ("mlp_opacity", "mlp_cov", "mlp_color")),
                      F=model.feat_dim, K=model.n_offsets)


class Scene(SimpleNamespace):
    """What ``load_scene`` returns: ``anchor [n, 3]`` (``get_anchor``'s values), ``anchor_feat [n, F]``, ``offset [n, K, 3]``,
    ``scaling [n, 6]``, ``mask [n, K, 1]``, ``bound_min``, ``bound_max`` ``[3]``, ``encoding`` (a ``MixEncoding`` whose tables
    hold +-1), ``mlp_grid``, ``mlps`` (name -> ``nn.Sequential``), ``F``, ``K``, ``n``."""

    def apply_to(self, model):
        """GM:1344-1368: replace the model's parameters by the decoded ones (``decoded_version = True``: ``get_anchor``
        and ``get_scaling`` then return ``_anchor`` and ``_scaling`` as they are)."""
        model._anchor_feat = nn.Parameter(self.anchor_feat)
        model._offset = nn.Parameter(self.offset)
        model.decoded_version = True
        model._anchor = nn.Parameter(self.anchor)
        model._scaling = nn.Parameter(self.scaling)
        model._mask = nn.Parameter(self.mask)
        model.x_bound_min, model.x_bound_max = self.bound_min.reshape(1, 3), self.bound_max.reshape(1, 3)
        for name in MixEncoding.NAMES:
            getattr(model.encoding_xyz, name).params = nn.Parameter(getattr(self.encoding, name).params.detach())
        for name, mlp in [(GRID_MLP, self.mlp_grid)] + list(self.mlps.items()):
            getattr(model, name).load_state_dict(mlp.state_dict())
        return model


class _Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, fmt):
        size = struct.calcsize(fmt)
        if self.at + size > len(self.data):
            raise ValueError("load_scene: a truncated file")
        out = struct.unpack_from(fmt, self.data, self.at)
        self.at += size
        return out

    def raw(self, size):
        if self.at + size > len(self.data):
            raise ValueError("load_scene: a truncated file")
        self.at += size
        return self.data[self.at - size:self.at]


@torch.no_grad()
def load_scene(path, device="cuda"):
    """The file alone -> ``Scene`` on ``device`` (a GPU: the decoders are kernels).  Raises ``ValueError`` for a file that is
    not one of this format, is truncated, or whose streams their decoders refuse."""
    who = "load_scene"
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: device must be a GPU (there is no CPU path)")
    with open(path, "rb") as f:
        data = f.read()
    r = _Reader(data)
    if r.raw(4) != MAGIC:
        raise ValueError(f"{who}: not a scene file (magic)")
    fmt, n, F, K = r.take("<4I")
    if fmt != FORMAT:
        raise ValueError(f"{who}: format {fmt} is not supported (this is {FORMAT})")
    # Nothing below is allocated from a number of the header before that number is bounded: by the kernels' own limits
    # and by the bytes of the section that has to hold it.
    if n > anchor_codec.MAX_N or not 1 <= F <= context.MAX_F or not 1 <= K <= context.MAX_K:
        raise ValueError(f"{who}: a corrupt header (n = {n}, F = {F}, K = {K})")
    n_features, log2_3d, log2_2d, l3, l2 = r.take("<5I")
    if n_features not in SUPPORTED_FEATURES or max(log2_3d, log2_2d) > MAX_LOG2_ROWS or not 1 <= l3 <= MAX_LEVELS \
            or not 1 <= l2 <= MAX_LEVELS or l3 + 3 * l2 > MAX_LEVELS:
        raise ValueError(f"{who}: a corrupt header (the encoding's arguments)")
    res3, res2 = list(r.take(f"<{l3}I")), list(r.take(f"<{l2}I"))
    if max(res3 + res2) > MAX_RESOLUTION or min(res3 + res2) < 1:
        raise ValueError(f"{who}: a corrupt header (the encoding's resolutions)")
    stacks = OrderedDict()
    (count,) = r.take("<I")
    if count < 1 or count > 64:
        raise ValueError(f"{who}: a corrupt header")
    for _ in range(count):
        (length,) = r.take("<I")
        name = bytes(r.raw(length + (-length % 4))[:length]).decode("utf-8")
        stacks[name] = r.take("<4I")
    (count,) = r.take("<I")
    if count != 10:
        raise ValueError(f"{who}: a corrupt header ({count} sections)")
    table = [r.take("<IQQ") for _ in range(count)]
    for kind, at, length in table:
        if kind not in SECTION_NAMES or at + length > len(data):
            raise ValueError(f"{who}: a truncated file")
    section = lambda kind: [data[at:at + length] for k, at, length in table if k == kind]
    kinds = [k for k, _, _ in table]
    if kinds != [SECTION_MLPS] + [SECTION_TABLE] * 4 + [SECTION_ANCHORS, SECTION_MASKS, SECTION_FEAT, SECTION_SCALING,
                                                        SECTION_OFFSETS] or GRID_MLP not in stacks:
        raise ValueError(f"{who}: a corrupt header (sections)")

    # 1. the MLPs
    blob = section(SECTION_MLPS)[0]
    for name, (d_in, hidden, d_out, code) in stacks.items():
        if code >= len(LAST_LAYERS) or min(d_in, hidden, d_out) < 1 or max(d_in, hidden, d_out) > MAX_WIDTH:
            raise ValueError(f"{who}: a corrupt header (the layers of {name})")
    if 4 * sum(h * (d + 1) + o * (h + 1) for d, h, o, _ in stacks.values()) != len(blob):
        raise ValueError(f"{who}: a corrupt file (the MLPs' widths do not add up to their section's {len(blob)} bytes)")
    raw = np.frombuffer(blob, dtype="<f4")
    mlps, at = OrderedDict(), 0
    for name, (d_in, hidden, d_out, code) in stacks.items():
        layers = [nn.Linear(d_in, hidden), nn.ReLU(True), nn.Linear(hidden, d_out)]
        layers += [LAST_LAYERS[code]()] if LAST_LAYERS[code] is not None else []
        mlp = nn.Sequential(*layers)
        for p in (layers[0].weight, layers[0].bias, layers[2].weight, layers[2].bias):
            if at + p.numel() > raw.size:
                raise ValueError(f"{who}: a truncated file (MLP parameters)")
            p.data = torch.from_numpy(raw[at:at + p.numel()].copy()).reshape(p.shape)
            at += p.numel()
        mlps[name] = mlp.to(device)
    mlp_grid = mlps.pop(GRID_MLP)
    # 2. the tables
    blobs = section(SECTION_TABLE)
    for name, blob, (dim, res, log2) in zip(MixEncoding.NAMES, blobs, [(3, res3, log2_3d)] + [(2, res2, log2_2d)] * 3):
        rows = table_offsets(dim, res, log2)[-1]          # (host arithmetic: nothing is allocated yet)
        if rows * n_features > MAX_SYMBOLS_PER_BYTE * len(blob):
            raise ValueError(f"{who}: a corrupt file (table {name} of {rows} rows in a section of {len(blob)} bytes)")
    encoding = MixEncoding(n_features, res3, log2_3d, res2, log2_2d)
    for name, blob in zip(MixEncoding.NAMES, blobs):
        params = getattr(encoding, name).params
        sym = _bernoulli_decode(who, f"table {name}", blob, device, params.numel())
        params.data = (sym.to(torch.float32) * 2 - 1).reshape(params.shape)
    encoding = encoding.to(device)
    # 3. the anchors
    blob = section(SECTION_ANCHORS)[0]
    if len(blob) < anchor_codec.HEADER_BYTES or n > 8 * len(blob):        # (an anchor costs a bit at the least)
        raise ValueError(f"{who}: a corrupt file ({n} anchors in a section of {len(blob)} bytes)")
    stream = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    anchor, bmin, bmax = anchor_codec.decode_anchors(stream, n=n, device=device)
    # 4. the masks
    blob = section(SECTION_MASKS)[0]
    if n * K > MAX_SYMBOLS_PER_BYTE * len(blob):
        raise ValueError(f"{who}: a corrupt file ({n} x {K} mask entries in a section of {len(blob)} bytes)")
    mask = _bernoulli_decode(who, "masks", blob, device, n * K)
    mask = mask.to(torch.float32).reshape(n, K, 1)
    # 5. - 7. the attributes, under the model of the decoded anchors and tables
    if n > 0:
        weights = _ops.sequential_weights(who, GRID_MLP, mlp_grid)
        _, ctx, Q = _model_operands(anchor, bmin, bmax, encoding, [w.detach() for w in weights], F, K)
        streams = [torch.frombuffer(bytearray(section(k)[0]), dtype=torch.uint8).to(device)
                   for k in (SECTION_FEAT, SECTION_SCALING, SECTION_OFFSETS)]
        feat, scaling, offset = codec.decode_attributes(streams, ctx, Q, mask, F, K)
    else:
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        feat, scaling, offset = z(0, F), z(0, 6), z(0, K, 3)
    return Scene(anchor=anchor, anchor_feat=feat, offset=offset, scaling=scaling, mask=mask, bound_min=bmin, bound_max=bmax,
                 encoding=encoding, mlp_grid=mlp_grid, mlps=mlps, F=F, K=K, n=n)
