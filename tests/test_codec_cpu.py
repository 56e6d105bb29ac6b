"""CPU tests of the entropy codec (include/bloomscene_codec.h, bloomscene_amd/codec.py, torchac/): the restatement of
tests/codec_reference.py round-trips exactly, its integer model is strictly increasing on adversarial operands, its Phi
holds the header's bound, its streams hold the size figures of docs/EXPERIMENTS.md; the library's entry points and the
python interface's checks -- all before the device is touched.  tests/test_codec_gpu.py compares the kernels' streams byte
for byte with the restatement's, so what is shown here of the streams binds the GPU's."""
import math
import os

import numpy as np
import pytest
import torch

import codec_reference as R
from bloomscene_amd import _capi
from bloomscene_amd import codec as Cd

f32 = np.float32


scene, requantised = R.scene, R.requantised


@pytest.mark.parametrize("n,C,spread,q,q_shape,T", [(37, 50, 1.0, 0.25, "scalar", 256), (400, 50, 1.0, 0.25, "row", 256),
                                                    (33, 30, 0.05, 0.25, "element", 4), (1, 63, 2.0, 0.05, "scalar", 1),
                                                    (2, 65, 0.3, 0.25, "row", 2)])
def test_restatement_round_trips_exactly(n, C, spread, q, q_shape, T):
    x, mean, scale, Q = scene(n, n, C, spread, q, q_shape)
    stream = R.encode_gaussian(x, mean, scale, Q, T=T)
    y = R.decode_gaussian(stream, mean, scale, Q)
    a, b = requantised(x, Q)
    assert (y.view(np.uint32) == a.view(np.uint32)).all() and (y == b).all()
    h = R.parse(stream)
    assert (h.magic, h.format, h.kind, h.elements, h.T) == (R.MAGIC, 1, 0, n * C, T)
    assert h.chunks == -(-n * C // (64 * T)) and stream.size == h.data + h.offsets[-1]


def test_restatement_round_trips_with_keep_and_the_table_model():
    x, mean, scale, Q = scene(5, 50, 30, 1.0, 0.05, "row")
    rng = np.random.default_rng(5)
    keep = (rng.random((50, 10)) < 0.6).astype(f32)
    keep[7] = 0
    stream = R.encode_gaussian(x, mean, scale, Q, keep=keep, keep_repeat=3, T=8)
    y = R.decode_gaussian(stream, mean, scale, Q, keep=keep, keep_repeat=3)
    a, b = requantised(x, Q, keep, 3)
    assert (y.view(np.uint32) == a.view(np.uint32)).all() and (y == b).all()
    # nothing kept: header only, zeros
    none = np.zeros_like(keep)
    stream = R.encode_gaussian(x, mean, scale, Q, keep=none, keep_repeat=3)
    assert stream.size == R.HEADER_BYTES and R.parse(stream).L == 0
    assert (R.decode_gaussian(stream, mean, scale, Q, keep=none, keep_repeat=3) == 0).all()
    # L == 1: header only, the one value
    one = np.full((3, 4), 0.26, f32)
    stream = R.encode_gaussian(one, one, one, f32(0.25))
    assert stream.size == R.HEADER_BYTES and R.parse(stream).L == 1 and R.parse(stream).kmin == 1
    assert (R.decode_gaussian(stream, one, one, f32(0.25)) == f32(0.25)).all()
    # the table model: one row, and a row per symbol
    for p in (1e-6, 0.5, 1 - 1e-6):
        sym = (rng.random(1000) < p).astype(np.int16)
        cdf = np.array([0, 1 - p, 1], f32)
        assert (R.decode_table(R.encode_table(sym, cdf, T=4), cdf, 1000) == sym).all()
    steps = np.sort(rng.random((300, 6)), axis=1).astype(f32)
    cdf = np.concatenate([np.zeros((300, 1), f32), steps, np.ones((300, 1), f32)], axis=1)
    sym = rng.integers(0, 7, 300).astype(np.int16)
    assert (R.decode_table(R.encode_table(sym, cdf, T=2), cdf, 300) == sym).all()
    with pytest.raises(R.Refused):
        R.encode_table(sym, cdf[:, ::-1].copy())


def test_restatement_refuses_what_the_header_refuses():
    x, mean, scale, Q = scene(9, 4, 5, 1.0, 0.25)
    for bad, status in ((np.nan, R.BAD_VALUE), (np.inf, R.BAD_VALUE), (1e12, R.BAD_VALUE)):
        xb = x.copy()
        xb[1, 2] = bad
        with pytest.raises(R.Refused) as e:
            R.encode_gaussian(xb, mean, scale, Q)
        assert e.value.status & status
    with pytest.raises(R.Refused) as e:
        R.encode_gaussian(x, mean, scale, f32(0))
    assert e.value.status & R.BAD_STEP
    mb = mean.copy()
    mb[0, 0] = np.inf
    with pytest.raises(R.Refused) as e:
        R.encode_gaussian(x, mb, scale, Q)
    assert e.value.status & R.BAD_MODEL
    xb = x.copy()
    xb[0, 0], xb[3, 4] = -5000.0, 5000.0
    with pytest.raises(R.Refused) as e:
        R.encode_gaussian(xb, mean, scale, Q)                      # a span of 40 001 steps
    assert e.value.status & R.BAD_SPAN
    stream = R.encode_gaussian(x, mean, scale, Q)
    wrong = stream.copy()
    wrong[0] ^= 1
    with pytest.raises(R.Refused) as e:
        R.decode_gaussian(wrong, mean, scale, Q)
    assert e.value.status & R.BAD_HEADER
    with pytest.raises(R.Refused) as e:
        R.decode_gaussian(stream[:-2], mean, scale, Q)
    assert e.value.status & R.TRUNCATED


ADVERSARIAL = {
    # name: (kmin, L, Q, [(mean, scale) rows])
    "point_mass": (-40, 81, 0.25, [(0.0, 1e-9), (0.13, 1e-9), (-10.0, 1e-9), (3.0, 1e-12)]),
    "wide": (-300, 601, 0.25, [(0.0, 10.0), (1.7, 10.0), (-60.0, 10.0)]),                # scale = 40 Q
    "mean_far_outside": (-20, 41, 0.25, [(1e4, 1.0), (-1e4, 0.3), (1e30, 5.0), (-3e38, 1.0), (40.0, 0.01)]),
    "two_symbols": (3, 2, 0.05, [(0.175, 0.01), (0.0, 1e-9), (0.2, 100.0), (-5.0, 1.0)]),
    "full_span": (-16383, 32767, 2.5e-4, [(0.0, 1.0), (0.0, 1e-9), (0.5, 1e-3), (-4.0, 0.05), (1e3, 1.0)]),
    "full_span_coarse": (-16383, 32767, 0.25, [(0.0, 500.0), (100.0, 4000.0), (0.0, 0.3)]),
}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_model_is_strictly_increasing_with_every_frequency_in_range(name):
    kmin, L, Q, rows = ADVERSARIAL[name]
    mean = np.array([[m] for m, _ in rows], f32)
    scale = np.array([[s] for _, s in rows], f32)
    model = R.gaussian_model(len(rows), 1, mean, scale, f32(Q), kmin, L)
    c = model.tables()
    assert c.shape == (len(rows), L + 1) and (c[:, 0] == 0).all() and (c[:, L] == 65536).all()
    f = np.diff(c, axis=1)
    assert (f >= 1).all() and (f <= 65535).all()
    if name == "point_mass":
        # the mass sits on one or two symbols; every other symbol is at the floor of 2
        assert ((f == 2).sum(axis=1) >= L - 2).all()


def test_table_model_is_strictly_increasing():
    rng = np.random.default_rng(0)
    for L in (2, 3, 255, 32767):
        steps = np.sort(rng.random((4, L - 1)), axis=1).astype(f32)
        cdf = np.concatenate([np.zeros((4, 1), f32), steps, np.ones((4, 1), f32)], axis=1)
        cdf[1, 1:-1] = 0.0          # all the mass on the last symbol
        cdf[2, 1:-1] = 1.0          # ... on the first
        f = np.diff(R.table_model(4, cdf).tables(), axis=1)
        assert (f >= 2).all() and (f <= 65535).all()


def test_phi_holds_its_bound():
    z = np.concatenate([np.linspace(-9, 9, 360001), np.linspace(-0.5, 0.5, 100001), [-np.inf, np.inf, -40.0, 40.0, 0.0, -0.0]])
    z = z.astype(f32)
    ref = np.array([0.5 * math.erfc(-float(v) / math.sqrt(2.0)) for v in z])
    P = R.phi(z)
    assert np.abs(P.astype(np.float64) - ref).max() <= 2e-7
    assert (P >= 0).all() and (P <= 1).all() and P[-6] == 0 and P[-5] == 1


SIZE_FIXTURES = {
    # name: (seed, n, C, spread, Q): 35 000 to 50 000 symbols, three or four chunks of 16 384 with a partial last one
    "wide": (1, 1000, 50, 1.0, 0.25),        # 3.3 bits a symbol
    "narrow": (2, 800, 50, 0.05, 0.25),      # 0.5 bits a symbol: probable symbols
    "fine": (3, 700, 50, 3.0, 0.05),         # 7.1 bits a symbol, L above 1000
}
# the figures of docs/EXPERIMENTS.md ("Entropy codec"), measured with the restatement on the fixtures above and on the
# three Bernoulli streams below: the largest coder loss, as a fraction of the ideal code length
MEASURED_CODER_LOSS = 0.0026


def _sizes(stream, ideal):
    """(stream bits, fixed bits, coder loss in bits).  The coder's own loss counts what the final states hold: a state x
    carries log2(x) - 16 bits of the symbols beyond the start state 2^16."""
    h = R.parse(stream)
    data = stream[h.data:]
    held = sum(float((np.log2(data[o:o + 256].view(np.uint32).astype(np.float64)) - 16).sum()) for o in h.offsets[:-1])
    fixed = 8 * R.fixed_bytes(stream)
    return 8 * stream.size, fixed, 8 * stream.size - fixed + held - ideal


def _size_cases():
    for name, (seed, n, C, spread, q) in sorted(SIZE_FIXTURES.items()):
        x, mean, scale, Q = scene(seed, n, C, spread, q)
        stream = R.encode_gaussian(x, mean, scale, Q)
        h = R.parse(stream)
        k, _ = R.symbols(x, np.full(n * C, Q, f32), n, C, np.ones(n * C, bool))
        yield name, stream, R.ideal_bits(R.gaussian_model(n, C, mean, scale, Q, h.kmin, h.L), k - h.kmin)
    for p in (0.1, 0.5, 1e-6):
        sym = (np.random.default_rng(7).random(50000) < p).astype(np.int16)
        cdf = np.array([0, 1 - p, 1], f32)
        yield f"bernoulli {p}", R.encode_table(sym, cdf), R.ideal_bits(R.table_model(50000, cdf), sym.astype(np.int64))


def test_stream_size_against_the_ideal_code_length():
    """The stream's bits against the ideal code length of the SAME integer model plus the format's fixed bytes (header,
    offsets, 256 B of final states a chunk).  Measured (docs/EXPERIMENTS.md): on every fixture the stream is SHORTER than
    ideal + fixed, by 0.03 % to 6.3 %, because the final states, counted as fixed, hold up to 16 bits of payload a lane;
    the coder's own loss (words + what the states hold - ideal) is at most 0.26 % of the ideal.  Asserted: the stream
    does not exceed ideal + fixed, and the coder's loss stays within twice the measured figure."""
    worst = 0.0
    for name, stream, ideal in _size_cases():
        bits, fixed, loss = _sizes(stream, ideal)
        print(f"{name}: stream {bits} bits, ideal {ideal:.1f}, fixed {fixed}, stream / (ideal + fixed) - 1 = "
              f"{bits / (ideal + fixed) - 1:+.5f}, coder loss / ideal = {loss / ideal:+.5f}")
        assert bits <= ideal + fixed, name
        assert loss <= 2 * MEASURED_CODER_LOSS * ideal, name
        worst = max(worst, loss / ideal)
    assert worst >= 0.5 * MEASURED_CODER_LOSS        # (the recorded figure is the one these fixtures give)


def test_entry_points_exist_and_size_their_buffers():
    lib = _capi.lib()
    for name in ("bsr_codec_encode_gaussian", "bsr_codec_decode_gaussian", "bsr_codec_encode_table", "bsr_codec_decode_table",
                 "bsr_codec_stream_bound", "bsr_codec_scratch_bytes"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    bound, scratch = lib.bsr_codec_stream_bound, lib.bsr_codec_scratch_bytes
    assert bound(0, 256) == 32 and scratch(0, 256) == 256
    # header, chunks + 1 offsets, 256 B a chunk, one word a symbol
    assert bound(1, 256) == 32 + 8 + 256 + 2 and bound(16385, 256) == 32 + 12 + 512 + 2 * 16385
    sizes = [0, 1, 63, 64, 65, 16383, 16384, 16385, 5_000_000]
    for T in (1, 4, 256):
        b = [bound(n, T) for n in sizes]
        s = [scratch(n, T) for n in sizes]
        assert all(x < y for x, y in zip(b, b[1:])) and all(x <= y for x, y in zip(s, s[1:])) and s[0] < s[-1]
        assert all(v % 256 == 0 for v in s)
        # the scratch holds every chunk's worst-case word area, its states and its count
        assert all(v >= -(-n // (64 * T)) * (128 * T + 256 + 4) for v, n in zip(s, sizes))
    assert bound(-1, 256) == 0 and bound(1, 0) == 0 and bound(1, 65537) == 0 and bound((1 << 30) + 1, 256) == 0
    assert bound(1 << 30, 1) == 0 and bound(1 << 30, 256) > 0        # (uint32 offsets)
    assert scratch(-1, 256) == 0 and scratch(1, 0) == 0


def test_entry_points_name_what_they_refuse_before_any_launch():
    """NULL and fake pointers only: a call that got as far as a launch would fail differently (there is no GPU here).
    (The error string belongs to the calling thread: the calls are made on one that dies with it.)"""
    import threading
    lib = _capi.lib()
    P = 4096          # never dereferenced on the host
    seen = []

    def refused(rc, *words):
        msg = _capi.last_error()
        seen.append((rc, all(w in msg for w in words), msg))

    def calls():
        enc, dec = lib.bsr_codec_encode_gaussian, lib.bsr_codec_decode_gaussian
        good = [4, 6, 3, P, 6, P, 6, P, 6, P, Cd.Q_ROW, P, 1e-9, 256, P, 1 << 20, P, P, None]

        def enc_with(**kw):
            names = ["n", "C", "r", "x", "xs", "mean", "ms", "scale", "ss", "q", "q_mode", "keep", "scale_min", "T", "stream",
                     "stream_bytes", "result", "scratch", "hip_stream"]
            args = list(good)
            for k, v in kw.items():
                args[names.index(k)] = v
            return enc(*args)

        refused(enc_with(n=-1), "bsr_codec_encode_gaussian", "n >= 0")
        refused(enc_with(r=4), "C % r")
        refused(enc_with(keep=None), "r must be 1 without keep")
        refused(enc_with(q_mode=3), "q_mode")
        refused(enc_with(ms=5), "ms 5")
        refused(enc_with(xs=2), "xs 2")
        refused(enc_with(x=None), "NULL x")
        refused(enc_with(mean=None), "NULL mean")
        refused(enc_with(scale=P + 2), "4-byte aligned")
        refused(enc_with(scale_min=0.0), "scale_min")
        refused(enc_with(T=0), "T must be")
        refused(enc_with(stream_bytes=100), "stream_bytes", "bsr_codec_stream_bound")
        refused(enc_with(stream=None), "NULL stream")
        refused(enc_with(scratch=P + 4), "scratch must be 8-byte aligned")
        refused(enc_with(n=1 << 20, C=1 << 11, r=1, keep=None, xs=1 << 11, ms=1 << 11, ss=1 << 11), "2^30")
        refused(dec(4, 6, 3, None, 100, P, 6, P, 6, P, Cd.Q_ROW, P, 1e-9, P, P, None), "bsr_codec_decode_gaussian", "NULL stream")
        refused(dec(4, 6, 3, P + 1, 100, P, 6, P, 6, P, Cd.Q_ROW, P, 1e-9, P, P, None), "stream and result must be 4-byte aligned")
        refused(dec(4, 6, 3, P, 100, P, 6, P, 6, P, Cd.Q_ROW, P, 1e-9, None, P, None), "NULL out")
        refused(lib.bsr_codec_encode_table(5, 0, P, P, 0, 256, P, 1 << 20, P, P, None), "bsr_codec_encode_table", "L must be")
        refused(lib.bsr_codec_encode_table(5, 40000, P, P, 0, 256, P, 1 << 20, P, P, None), "L must be")
        refused(lib.bsr_codec_encode_table(5, 2, P, P, 2, 256, P, 1 << 20, P, P, None), "cs must be")
        refused(lib.bsr_codec_encode_table(5, 2, None, P, 0, 256, P, 1 << 20, P, P, None), "NULL sym")
        refused(lib.bsr_codec_decode_table(5, 2, P, 100, None, 0, P, P, None), "bsr_codec_decode_table", "NULL cdf")
        refused(lib.bsr_codec_decode_table(5, 2, P, 100, P, 0, None, P, None), "NULL out")
        refused(lib.bsr_codec_decode_table(-1, 2, P, 100, P, 0, P, P, None), "n must be")

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert len(seen) == 25 and all(rc == 1 and ok for rc, ok, _ in seen), [m for m in seen if not (m[0] == 1 and m[1])]


def test_python_checks_keep_the_siblings_order():
    """TypeError for a wrong dtype first, then NotImplementedError, then the shapes (ValueError), the device last."""
    n, C = 6, 9
    x, mean, scale = torch.zeros(n, C), torch.zeros(n, C), torch.ones(n, C)
    keep = torch.ones(n, 3)
    stream = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(TypeError, match="x must be float32"):
        Cd.encode_gaussian(x.double(), mean[:2], scale, 0.25)                  # (a wrong shape as well: the dtype wins)
    with pytest.raises(TypeError, match="scale must be float32"):
        Cd.encode_gaussian(x.reshape(3, 2, 9), mean, scale.half(), 0.25)
    with pytest.raises(TypeError, match="Q must be"):
        Cd.encode_gaussian(x, mean, scale, "0.25")
    with pytest.raises(TypeError, match="mean must be a torch.Tensor"):
        Cd.encode_gaussian(x, mean.numpy(), scale, 0.25)
    with pytest.raises(TypeError, match="stream must be uint8"):
        Cd.decode_gaussian(stream.float(), mean, scale, 0.25)
    with pytest.raises(NotImplementedError, match="3 dimensions"):
        Cd.encode_gaussian(x.reshape(3, 2, 9), mean[:2], scale, 0.25)          # (wrong shapes as well)
    with pytest.raises(ValueError, match=r"mean must be \[6, 9\]"):
        Cd.encode_gaussian(x, mean[:2], scale, 0.25)
    with pytest.raises(ValueError, match="keep_repeat must divide"):
        Cd.encode_gaussian(x, mean, scale, 0.25, keep=keep, keep_repeat=2)
    with pytest.raises(ValueError, match="without keep"):
        Cd.encode_gaussian(x, mean, scale, 0.25, keep_repeat=3)
    with pytest.raises(ValueError, match="Q must be a scalar"):
        Cd.encode_gaussian(x, mean, scale, torch.ones(n, 2))
    with pytest.raises(ValueError, match=r"keep must be \[6, 3\]"):
        Cd.encode_gaussian(x, mean, scale, 0.25, keep=torch.ones(n, 4), keep_repeat=3)
    with pytest.raises(ValueError, match="scale_min"):
        Cd.encode_gaussian(x, mean, scale, 0.25, scale_min=0.0)
    with pytest.raises(ValueError, match="must be on the GPU"):
        Cd.encode_gaussian(x, mean, scale, 0.25, keep=keep, keep_repeat=3)
    with pytest.raises(ValueError, match="must be on the GPU"):
        Cd.decode_gaussian(stream, mean, scale, 0.25)
    with pytest.raises(ValueError, match="must be on the GPU"):
        Cd.encode_gaussian(x[:, 0], mean[:, 0], scale[:, 0], torch.ones(n))   # (the drop-ins' 1-D form)
    # the table model
    sym, cdf = torch.zeros(5, dtype=torch.int16), torch.tensor([0.0, 0.5, 1.0])
    with pytest.raises(TypeError, match="sym must be int16"):
        Cd.encode_symbols(sym.long(), cdf[:1])
    with pytest.raises(TypeError, match="cdf must be float32"):
        Cd.encode_symbols(sym, cdf.double())
    with pytest.raises(NotImplementedError, match="3 dimensions"):
        Cd.encode_symbols(sym, cdf.reshape(1, 1, 3))
    with pytest.raises(ValueError, match="columns"):
        Cd.encode_symbols(sym, cdf[:1])
    with pytest.raises(ValueError, match="one row per symbol"):
        Cd.encode_symbols(sym, cdf.repeat(4, 1))
    with pytest.raises(ValueError, match="must be on the GPU"):
        Cd.encode_symbols(sym, cdf)
    with pytest.raises(ValueError, match="must be on the GPU"):
        Cd.decode_symbols(stream, cdf, 5)
    with pytest.raises(ValueError, match=r"context must be \[n, 175\]"):
        Cd.encode_attributes(torch.zeros(4, 170), torch.ones(4, 3), None, None, None, None, 50, 10)


def test_torchac_shim_resolves_without_a_gpu():
    import torchac
    assert callable(torchac.encode_float_cdf) and callable(torchac.decode_float_cdf)
    with pytest.raises(NotImplementedError):
        torchac.encode_int16_normalized_cdf(None, None)
    with pytest.raises(NotImplementedError):
        torchac.some_other_name()
    with pytest.raises(TypeError, match="cdf_float must be float32"):
        torchac.encode_float_cdf(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int16))
    with pytest.raises(TypeError, match="sym must be int16"):
        torchac.encode_float_cdf(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="sym must be"):
        torchac.encode_float_cdf(torch.zeros(4, 3), torch.zeros(5, dtype=torch.int16))
    with pytest.raises(TypeError, match="byte_stream must be bytes"):
        torchac.decode_float_cdf(torch.zeros(4, 3), torch.zeros(4))
    # the constants python restates are the header's
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bloomscene_codec.h")).read()
    for name, value in (("BSR_CODEC_DEFAULT_STEPS", Cd.DEFAULT_STEPS), ("BSR_CODEC_MAX_SYMBOLS", Cd.MAX_SYMBOLS),
                        ("BSR_CODEC_HEADER_BYTES", Cd.HEADER_BYTES), ("BSR_CODEC_FORMAT", R.FORMAT)):
        assert f"#define {name} {value}" in hdr
    assert f"#define BSR_CODEC_MAGIC {R.MAGIC:#x}u" in hdr
    for bit, name in enumerate(("VALUE", "STEP", "MODEL", "SPAN", "TABLE", "SYMBOL")):
        assert f"#define BSR_CODEC_BAD_{name} {1 << bit}u" in hdr
    assert len(Cd.STATUS) == 9 and "#define BSR_CODEC_CORRUPT 256u" in hdr
