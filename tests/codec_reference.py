"""CPU restatement of the entropy codec (include/bloomscene_codec.h, bloomscene_amd/codec.py) in numpy: the pinned ``Phi``,
the integer model ``c(j)`` of both models, the chunked interleaved rANS coder and the stream layout, bit for bit what the
kernels compute -- the GPU test compares streams byte for byte.

Vectorised over the 64 lanes of a step AND over the chunks: the coder's loop runs over the T steps of all chunks at once
(integer work only in the encoder, whose model values are taken for every element beforehand; ``ceil(log2 L)`` model
evaluations a step in the decoder), so a chunk of 16 384 symbols takes well under a second.

    stream = encode_gaussian(x, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9, T=256)   # uint8 array
    y = decode_gaussian(stream, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9)          # [n, C] float32
    stream = encode_table(sym, cdf, T=256);  sym = decode_table(stream, cdf, n)
    gaussian_model(...) / table_model(...) -> Model: c(idx, j), and tables(): the whole [elements, L + 1] integer table
    ideal_bits(model, j), fixed_bytes(stream)
    scene(seed, n, C, spread, q, q_shape), requantised(x, Q, keep, r): seeded operands and the expected decode
"""
from types import SimpleNamespace

import numpy as np

from heads_reference import fma32

MAGIC, FORMAT, HEADER_BYTES = 0x43525342, 1, 32
KIND_GAUSSIAN, KIND_TABLE = 0, 1
MAX_SYMBOLS = 32767
BAD_VALUE, BAD_STEP, BAD_MODEL, BAD_SPAN, BAD_TABLE, BAD_SYMBOL, BAD_HEADER, TRUNCATED, CORRUPT = (1 << b for b in range(9))
f32 = np.float32


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"codec status {status:#x}")
        self.status = status


def expf32(x):
    """bsr_expf of csrc/common.h for x <= 0 (no NaN): 0 below -104."""
    x = np.asarray(x, f32)
    live = x >= f32(-104.0)
    xs = np.where(live, x, f32(0))
    k = np.rint(xs * f32(1.44269504088896341)).astype(f32)
    r = fma32(-k, f32(0.693359375), xs)
    r = fma32(-k, f32(-2.12194440e-4), r)
    p = np.full_like(r, f32(1.0 / 5040.0))
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        p = fma32(p, r, f32(c))
    return np.where(live, np.ldexp(p, k.astype(np.int32)).astype(f32), f32(0))


def phi(z):
    """The header's Phi, operation by operation in fp32."""
    z = np.asarray(z, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.abs(z) * f32(0.70710678118654752440)
        a = np.where(a > f32(16.0), f32(16.0), a)
        w = f32(0.3275911) * a
        u = w / (f32(1.0) + w)
        p = f32(-1.061405429) * u + f32(3.853875118)
        p = p * u + f32(-6.222859923)
        p = p * u + f32(5.874886615)
        p = p * u + f32(-3.44449638)
        p = p * u + f32(1.0)
        h = f32(0.5) * (p * expf32(-(a * a)))
    return np.where(z < 0, h, f32(1.0) - h).astype(f32)


class Model:
    """c(idx, j): the integer cdf of the elements ``idx`` (flat indices of the coded order) at the symbols ``j``."""

    def __init__(self, kind, elements, active, kmin, L, value):
        self.kind, self.elements, self.active, self.kmin, self.L, self._value = kind, elements, active, kmin, L, value

    def c(self, idx, j):
        idx, j = np.broadcast_arrays(np.asarray(idx), np.asarray(j))
        L = self.L
        inner = np.clip(j, 1, max(L - 1, 1))
        P = self._value(idx, inner)
        with np.errstate(invalid="ignore"):
            mid = np.rint(P * f32(65536 - 2 * L)).astype(np.int64) + 2 * inner
        return np.where(j <= 0, 0, np.where(j >= L, 65536, mid)).astype(np.int64)

    def tables(self):
        """[elements, L + 1]: every c of every element (small cases only)."""
        idx = np.arange(self.elements)[:, None]
        return self.c(idx, np.arange(self.L + 1)[None, :])


def _flat_operands(n, C, mean, scale, Q, keep, keep_repeat, scale_min):
    mean = np.ascontiguousarray(mean, f32).reshape(n * C)
    scale = np.ascontiguousarray(scale, f32).reshape(n * C)
    Q = np.asarray(Q, f32)
    if Q.size == 1:
        q = np.full(n * C, Q.reshape(()), f32)
    elif Q.size == n:
        q = np.repeat(Q.reshape(n), C)
    else:
        q = Q.reshape(n * C)
    if keep is None:
        active = np.ones(n * C, bool)
    else:
        active = np.repeat(np.asarray(keep, f32).reshape(n, C // keep_repeat) != 0, keep_repeat, axis=1).reshape(n * C)
    status = 0
    if (~((q > 0) & np.isfinite(q)) & active).any():
        status |= BAD_STEP
    if (~(np.isfinite(mean) & np.isfinite(scale)) & active).any():
        status |= BAD_MODEL
    s = np.where(scale < f32(scale_min), f32(scale_min), scale).astype(f32)
    return mean, s, q, active, status


def gaussian_model(n, C, mean, scale, Q, kmin, L, keep=None, keep_repeat=1, scale_min=1e-9):
    mean, s, q, active, status = _flat_operands(n, C, mean, scale, Q, keep, keep_repeat, scale_min)
    if status:
        raise Refused(status)

    def value(idx, j):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            z = (((kmin + j).astype(f32) - f32(0.5)) * q[idx] - mean[idx]) / s[idx]
        return phi(z)

    m = Model(KIND_GAUSSIAN, n * C, active, kmin, L, value)
    m.q = q
    return m


def table_status(cdf):
    cdf = np.asarray(cdf, f32)
    cdf = cdf.reshape(-1, cdf.shape[-1])
    with np.errstate(invalid="ignore"):
        ok = (cdf[:, :-1] >= 0) & (cdf[:, :-1] <= cdf[:, 1:]) & (cdf[:, 1:] <= 1)
    return 0 if ok.all() else BAD_TABLE


def table_model(n, cdf):
    cdf = np.asarray(cdf, f32)
    rows = cdf.reshape(-1, cdf.shape[-1])
    L = rows.shape[1] - 1
    one = rows.shape[0] == 1 and cdf.ndim == 1

    def value(idx, j):
        return rows[np.zeros_like(idx) if one else idx, j]

    return Model(KIND_TABLE, n, np.ones(n, bool), 0, L, value)


def symbols(x, Q, n, C, active):
    """k = rint(x / Q) of the header -> (k int64 [n C], status)."""
    x = np.ascontiguousarray(x, f32).reshape(n * C)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        k = np.rint(x / Q)
    bad = ~(np.abs(k) < 2.0 ** 30) & active
    return np.where(active & ~bad, k, 0).astype(np.int64), (BAD_VALUE if bad.any() else 0)


def _header(kind, elements, kmin, L, T, chunks):
    return np.array([MAGIC, FORMAT, kind, elements, kmin & 0xffffffff, L, T, chunks], np.uint32)


def _chunk_grid(elements, T):
    chunks = -(-elements // (64 * T))
    return chunks, chunks * 64 * T


def encode(model, j, T=256):
    """The coder and the layout: ``j`` int [elements] (ignored where the model is not active) -> uint8 stream."""
    n, L = model.elements, model.L
    if L < 2 or n == 0:
        return _header(model.kind, n, model.kmin, L, T, 0).view(np.uint8)
    chunks, padded = _chunk_grid(n, T)
    idx = np.arange(n)
    b = model.c(idx, j)
    f = model.c(idx, j + 1) - b

    def grid(v, fill):
        out = np.full(padded, fill, v.dtype)
        out[:n] = v
        return out.reshape(chunks, T, 64)

    B, F, A = grid(b, 0), grid(f, 1), grid(model.active, False)
    x = np.full((chunks, 64), 1 << 16, np.int64)
    W = np.zeros((chunks, T, 64), np.uint16)
    E = np.zeros((chunks, T, 64), bool)
    for s in range(T - 1, -1, -1):
        fs, bs, act = F[:, s], B[:, s], A[:, s]
        emit = act & (x >= (fs << 16))
        W[:, s] = np.where(emit, x & 0xffff, 0)
        E[:, s] = emit
        x = np.where(emit, x >> 16, x)
        x = np.where(act, ((x // fs) << 16) + (x % fs) + bs, x)
    parts, offsets = [], [0]
    for c in range(chunks):
        words = W[c][E[c]]                      # (step, lane) order: the decoder's
        parts.append(x[c].astype(np.uint32).view(np.uint8))
        parts.append(words.astype(np.uint16).view(np.uint8))
        offsets.append(offsets[-1] + 256 + 2 * words.size)
    head = np.concatenate([_header(model.kind, n, model.kmin, L, T, chunks), np.array(offsets, np.uint32)]).view(np.uint8)
    return np.concatenate([head] + parts)


def parse(stream):
    """-> the header's fields, the offsets and the byte position of the chunk data (no checks beyond the sizes)."""
    stream = np.ascontiguousarray(stream, np.uint8)
    if stream.size < HEADER_BYTES:
        raise Refused(TRUNCATED)
    h = stream[:HEADER_BYTES].view(np.uint32)
    out = SimpleNamespace(magic=int(h[0]), format=int(h[1]), kind=int(h[2]), elements=int(h[3]),
                          kmin=int(h[4:5].view(np.int32)[0]), L=int(h[5]), T=int(h[6]), chunks=int(h[7]))
    out.data = HEADER_BYTES + (4 * (out.chunks + 1) if out.chunks else 0)
    if stream.size < out.data:
        raise Refused(TRUNCATED)
    out.offsets = stream[HEADER_BYTES:out.data].view(np.uint32).astype(np.int64)
    return out


def decode(stream, make_model, kind, elements, table_L=None):
    """``make_model(kmin, L)`` -> Model.  -> (j int64 [elements], active, model); raises Refused with the status bits."""
    stream = np.ascontiguousarray(stream, np.uint8)
    h = parse(stream)
    ok = (h.magic == MAGIC and h.format == FORMAT and h.kind == kind and h.elements == elements and h.L <= MAX_SYMBOLS
          and 1 <= h.T <= 65536)
    if ok:
        want = -(-elements // (64 * h.T)) if h.L >= 2 else 0
        ok = h.chunks == want and (elements > 0 or h.L == 0)
        if kind == KIND_TABLE:
            ok = ok and (elements == 0 if h.L == 0 else h.L == table_L) and h.kmin == 0
    if not ok:
        raise Refused(BAD_HEADER)
    model = make_model(h.kmin, h.L)
    if h.L < 2:
        return np.zeros(elements, np.int64), model.active & (h.L == 1), model
    T, L, chunks = h.T, h.L, h.chunks
    padded = chunks * 64 * T
    data = stream[h.data:]
    status = 0
    sizes = np.diff(h.offsets)
    if (sizes < 256).any() or (h.offsets % 2).any():
        raise Refused(CORRUPT)
    if h.offsets[-1] > data.size:
        raise Refused(TRUNCATED)
    nwords = (sizes - 256) // 2
    x = np.zeros((chunks, 64), np.int64)
    words = np.zeros((chunks, int(nwords.max()) + 64), np.int64)
    for c in range(chunks):
        o = int(h.offsets[c])
        x[c] = data[o:o + 256].view(np.uint32)
        words[c, :nwords[c]] = data[o + 256:o + 256 + 2 * nwords[c]].view(np.uint16)
    A = np.zeros(padded, bool)
    A[:elements] = model.active
    A = A.reshape(chunks, T, 64)
    I = np.minimum(np.arange(padded), elements - 1).reshape(chunks, T, 64)
    J = np.zeros((chunks, T, 64), np.int64)
    trips = int(np.ceil(np.log2(L)))
    nxt = np.zeros(chunks, np.int64)
    for s in range(T):
        act, idx = A[:, s], I[:, s]
        if not act.any():
            continue
        v = x & 0xffff
        lo, hi = np.zeros_like(x), np.full_like(x, L)
        clo, chi = np.zeros_like(x), np.full_like(x, 65536)
        for _ in range(trips):
            mid = (lo + hi) >> 1
            cm = model.c(idx, mid)
            left = cm <= v
            lo, clo = np.where(left, mid, lo), np.where(left, cm, clo)
            hi, chi = np.where(left, hi, mid), np.where(left, chi, cm)
        x = np.where(act, (chi - clo) * (x >> 16) + v - clo, x)
        take = act & (x < (1 << 16))
        rank = np.cumsum(take, axis=1) - take
        at = nxt[:, None] + rank
        if (take & (at >= nwords[:, None])).any():
            status |= TRUNCATED
        w = np.take_along_axis(words, np.minimum(at, words.shape[1] - 1), axis=1)
        x = np.where(take, ((x << 16) | w) & 0xffffffff, x)
        nxt = nxt + take.sum(axis=1)
        J[:, s] = np.where(act, lo, 0)
    if (x != (1 << 16)).any() or (nxt != nwords).any():
        status |= CORRUPT
    if status:
        raise Refused(status)
    return J.reshape(padded)[:elements], model.active, model


# ---- the four functions of bloomscene_amd/codec.py ----
def encode_gaussian(x, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9, T=256):
    x = np.asarray(x, f32)
    n, C = x.shape
    mean_f, s, q, active, status = _flat_operands(n, C, mean, scale, Q, keep, keep_repeat, scale_min)
    k, bad = symbols(x, q, n, C, active)
    status |= bad
    if active.any() and not status:
        kmin, kmax = int(k[active].min()), int(k[active].max())
        L = kmax - kmin + 1
        if L > MAX_SYMBOLS:
            status |= BAD_SPAN
    else:
        kmin, L = 0, 0
    if status:
        raise Refused(status)
    model = gaussian_model(n, C, mean, scale, Q, kmin, L, keep, keep_repeat, scale_min)
    return encode(model, k - kmin, T)


def decode_gaussian(stream, mean, scale, Q, keep=None, keep_repeat=1, scale_min=1e-9):
    mean = np.asarray(mean, f32)
    n, C = mean.shape
    j, coded, model = decode(stream, lambda kmin, L: gaussian_model(n, C, mean, scale, Q, kmin, L, keep, keep_repeat, scale_min),
                             KIND_GAUSSIAN, n * C)
    y = (j + model.kmin).astype(f32) * model.q
    return np.where(coded, y, f32(0)).astype(f32).reshape(n, C)


def encode_table(sym, cdf, T=256):
    sym = np.asarray(sym, np.int64).reshape(-1)
    model = table_model(sym.size, cdf)
    status = table_status(cdf) | (BAD_SYMBOL if ((sym < 0) | (sym >= model.L)).any() else 0)
    if status:
        raise Refused(status)
    if sym.size == 0:
        model.L = 0
    return encode(model, sym, T)


def decode_table(stream, cdf, n):
    if table_status(cdf):
        raise Refused(BAD_TABLE)
    L = np.asarray(cdf).shape[-1] - 1

    def make(kmin, Lh):
        m = table_model(n, cdf)
        m.L = Lh
        return m

    j, _, _ = decode(stream, make, KIND_TABLE, n, table_L=L)
    return j.astype(np.int16)


# ---- sizes ----
def ideal_bits(model, j):
    """sum of -log2((c(j + 1) - c(j)) / 65536) over the active elements: the code length of the SAME integer model."""
    idx = np.arange(model.elements)
    f = (model.c(idx, j + 1) - model.c(idx, j))[model.active]
    return float(-np.log2(f / 65536.0).sum())


def fixed_bytes(stream):
    """The format's own bytes in a stream: header, offset table and 256 B of final states per chunk."""
    h = parse(stream)
    return h.data + 256 * h.chunks


# ---- what the tests share ----
def scene(seed, n, C, spread, q, q_shape="scalar"):
    """Seeded operands: means of order 1, scales around ``spread``, x drawn from the model."""
    rng = np.random.default_rng(seed)
    mean = rng.normal(0, 1, (n, C)).astype(f32)
    scale = (np.abs(rng.normal(0, 1, (n, C))) * spread + 0.01).astype(f32)
    x = (mean + scale * rng.normal(0, 1, (n, C))).astype(f32)
    if q_shape == "scalar":
        Q = f32(q)
    elif q_shape == "row":
        Q = (q * (1 + 0.5 * np.tanh(rng.normal(0, 1, (n, 1))))).astype(f32)
    else:
        Q = (q * (1 + 0.5 * np.tanh(rng.normal(0, 1, (n, C))))).astype(f32)
    return x, mean, scale, Q


def requantised(x, Q, keep=None, r=1):
    """(the header's decoded value float(k) * Q, and rint(x / Q) * Q: equal as numbers, and bit for bit apart from a
    zero's sign -- rint gives -0 for a small negative x, an integer has no -0)"""
    n, C = x.shape
    Qb = np.broadcast_to(np.asarray(Q, f32).reshape(-1, 1) if np.asarray(Q).size == n else np.asarray(Q, f32), (n, C))
    k = np.rint(x / Qb)
    a, b = (k.astype(np.int64).astype(f32) * Qb).astype(f32), (k * Qb).astype(f32)
    if keep is not None:
        m = np.repeat(np.asarray(keep).reshape(n, C // r) != 0, r, axis=1)
        a, b = np.where(m, a, f32(0)), np.where(m, b, f32(0))
    return a, b
