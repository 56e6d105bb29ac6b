"""CPU tests of the anchor position coder (include/bloomscene_anchor_codec.h, bloomscene_amd/anchor_codec.py): the numpy
restatement of tests/anchor_codec_reference.py round-trips, its lattice is torch's floor division, its decoded anchors are
Quantize_anchor's bit for bit, its stream is below the reference's reported 48 bits an anchor on a stated scene; the
library's sizing entry points and the python interface's checks -- all before the device is touched.
tests/test_anchor_codec_gpu.py compares the kernels' streams byte for byte with the restatement's, so what is shown here of
the streams binds the GPU's."""
import struct

import numpy as np
import pytest
import torch

import anchor_codec_reference as R
from anchor_state_reference import Q_ANCHOR
from bloomscene_amd import _capi
from bloomscene_amd import anchor_codec as AC

f32 = np.float32
BMIN, BMAX = np.array([-1.5, -0.75, 0.25], f32), np.array([2.5, 1.25, 3.0], f32)


def random_anchors(n, seed, lo=-0.1, hi=1.1):
    rng = np.random.default_rng(seed)
    return (BMIN + (BMAX - BMIN) * rng.uniform(lo, hi, (n, 3))).astype(f32)


def adversarial_inputs():
    """(name, anchor [n, 3], bmin, bmax): exact multiples of the interval, max == min, values outside the bounds."""
    rng = np.random.default_rng(3)
    interval = R.interval_np(BMIN, BMAX)
    exact = ((rng.integers(0, 65536, (4000, 3)).astype(f32) * interval).astype(f32) + BMIN).astype(f32)
    edge = np.concatenate([np.nextafter(exact[:500], f32(np.inf)), np.nextafter(exact[:500], f32(-np.inf))]).astype(f32)
    flat = np.array([0.5, 0.5, 0.5], f32)
    return [("random", random_anchors(5000, 1), BMIN, BMAX), ("exact multiples", exact, BMIN, BMAX),
            ("one ulp beside a multiple", edge, BMIN, BMAX),
            ("max == min", (flat + rng.uniform(-1e-3, 1e-3, (2000, 3))).astype(f32), flat, flat),
            ("outside the bounds", random_anchors(3000, 2, -3.0, 4.0), BMIN, BMAX)]


def torch_lattice(anchor, bmin, bmax):
    """utils/encodings.py:215-227 up to the clamp, on CPU torch."""
    a, lo, hi = (torch.from_numpy(np.asarray(t, f32)) for t in (anchor, bmin.reshape(1, 3), bmax.reshape(1, 3)))
    interval = (hi - lo) * Q_ANCHOR + 1e-6
    q = torch.clamp(torch.div(a - lo, interval, rounding_mode="floor"), 0, 2 ** 16 - 1)
    return q, q * interval + lo


@pytest.mark.parametrize("case", adversarial_inputs(), ids=lambda c: c[0])
def test_lattice_is_torch_floor_division_and_the_decoded_anchor_is_quantize_anchor(case):
    _, anchor, bmin, bmax = case
    q, dequantised = torch_lattice(anchor, bmin, bmax)
    mine = R.lattice_np(anchor, bmin, bmax)
    assert (mine == q.numpy()).all()
    keys = R.keys_np(anchor, bmin, bmax)
    got = R.dequantise_np(keys, bmin, bmax)
    assert (got.view(np.uint32) == dequantised.numpy().view(np.uint32)).all()
    assert ((keys >> np.uint64(32)) == mine[:, 0].astype(np.uint64)).all() and int(keys.max()) < 1 << 48


def key_sets():
    rng = np.random.default_rng(11)
    top = (1 << 48) - 1
    near = np.sort(rng.integers(0, 1 << 20, 300))
    return {
        "n = 0": [], "n = 1": [12345], "n = 2": [5, 1 << 40], "all equal": [777] * 300,
        "0 and 2^48 - 1 (k = 47)": [0, top],
        "chunk edges": np.sort(rng.integers(0, 1 << 48, 513)).tolist(),
        "two clusters in a chunk (the escape)": np.concatenate([near, near + (1 << 45)]).tolist()[100:400],
        "duplicates across a chunk edge": np.sort(np.repeat(rng.integers(0, 1 << 30, 130), 4)).tolist(),
        "dense": np.sort(rng.integers(0, 4000, 1000)).tolist(),
    }


@pytest.mark.parametrize("name", list(key_sets()))
def test_restatement_round_trips(name):
    keys = key_sets()[name]
    stream = R.encode_keys(keys, BMIN, BMAX)
    got, anchor, bmin, bmax = R.decode_np(stream)
    assert got.tolist() == keys and (bmin == BMIN).all() and (bmax == BMAX).all()
    assert (anchor.view(np.uint32) == R.dequantise_np(np.array(keys, np.uint64), BMIN, BMAX).view(np.uint32)).all()
    n, chunks = struct.unpack("<2I", stream[8:16])
    assert (n, chunks) == (len(keys), -(-len(keys) // 256))
    assert len(stream) <= 48 + (4 * (chunks + 1) if chunks else 0) + 2560 * chunks


def test_restatement_layout_by_hand():
    """Three keys, gaps 5 and 40: mean = 22, k = 4.  5 = 0 * 16 + 5: '0' then 0101 lowest first; 40 = 2 * 16 + 8: '110' then
    1000 lowest first.  Bits, first to last: 0 1010 110 0001 -> as a number 0b1000_011_0101_0 = 0x86a."""
    stream = R.encode_keys([100, 105, 145], BMIN, BMAX)
    assert len(stream) == 48 + 8 + 8 + 4
    assert struct.unpack("<2I", stream[48:56]) == (0, 12)
    assert struct.unpack("<QI", stream[56:]) == (100 | 4 << 48, 0x86a)
    # the escape: gaps 0 and 2^40 with mean 2^39, k = 39: 2^40 >> 39 = 2 is no escape; gaps 0 (x 40) and 2^40: mean 2^40 / 41
    keys = [0] * 41 + [1 << 40]
    k = ((1 << 40) // 41).bit_length() - 1
    assert (1 << 40) >> k >= 32
    stream = R.encode_keys(keys, BMIN, BMAX)
    bits = int.from_bytes(stream[48 + 8 + 8:], "little")
    assert bits == ((1 << 32) - 1 | (1 << 40) << 32) << 40 * (1 + k)


def test_restatement_refuses_what_the_header_lists():
    keys = np.sort(np.random.default_rng(5).integers(0, 1 << 30, 600)).tolist()
    stream = R.encode_keys(keys, BMIN, BMAX)
    table = 48 + 4 * 4
    for cut, what in ((20, "truncated"), (48 + 6, "truncated"), (table + 100, "truncated")):
        with pytest.raises(ValueError, match=what):
            R.decode_np(stream[:cut])
    swapped = bytearray(stream)
    swapped[52:56], swapped[56:60] = stream[56:60], stream[52:56]
    with pytest.raises(ValueError, match="corrupt"):
        R.decode_np(swapped)
    for at, value in ((0, 0), (4, 2), (16, 128), (20, 16), (12, 2), (8, 1000)):
        bad = bytearray(stream)
        bad[at:at + 4] = struct.pack("<I", value)
        with pytest.raises(ValueError, match="not a stream"):
            R.decode_np(bad)
    # all gaps 0 (k = 0, one zero bit each): a flipped byte is one gap of 8 in 9 bits where 8 gaps took 8, so the 255 gaps
    # need 263 bits of the chunk's 256
    flat = bytearray(R.encode_keys([9] * 256, BMIN, BMAX))
    assert len(flat) == 48 + 8 + 8 + 32
    flat[48 + 8 + 8 + 5] ^= 0xff
    with pytest.raises(ValueError, match="corrupt"):
        R.decode_np(flat)
    with pytest.raises(ValueError, match="ascending"):
        R.encode_keys([2, 1], BMIN, BMAX)
    with pytest.raises(ValueError, match="2\\^48"):
        R.encode_keys([1, 1 << 48], BMIN, BMAX)
    with pytest.raises(ValueError, match="non-finite"):
        R.keys_np(np.array([[0.0, np.nan, 0.0]], f32), BMIN, BMAX)


def test_order_is_ascending_key_then_source_row():
    anchor = random_anchors(700, 9)
    anchor[100:140] = anchor[300:340]                                # duplicated rows
    rows = np.sort(np.random.default_rng(2).choice(700, 500, replace=False))
    for r in (None, rows, np.isin(np.arange(700), rows)):
        stream, perm = R.encode_np(anchor, BMIN, BMAX, r)
        keys = R.keys_np(anchor, BMIN, BMAX)[perm]
        assert (np.diff(keys.astype(np.int64)) >= 0).all()
        same = np.diff(keys.astype(np.int64)) == 0
        assert same.any() and (np.diff(perm)[same] > 0).all()
        assert (R.decode_np(stream)[0] == keys).all()


def test_size_condition_surface_scene_is_below_the_reported_48_bits():
    """The scene of anchor_codec_reference.surface_scene(200 000 points, voxel 0.01, seed 0): points on five surfaces,
    voxelised as anchor creation does, bounds by update_anchor_bound.  The reference REPORTS 48 bits an anchor
    (scene/gaussian_model.py:1049) and writes 96."""
    anchor, bmin, bmax = R.surface_scene()
    n = anchor.shape[0]
    assert n >= 20000
    stream, perm = R.encode_np(anchor, bmin, bmax)
    bits = 8 * len(stream) / n
    print(f"surface scene: {n} anchors, {len(stream)} bytes, {bits:.2f} bits per anchor")
    assert bits < 48
    keys, decoded, _, _ = R.decode_np(stream)
    _, want = torch_lattice(anchor[perm], bmin, bmax)
    assert (decoded.view(np.uint32) == want.numpy().view(np.uint32)).all()


def test_sizing_entry_points_and_constants():
    lib = _capi.lib()
    assert lib.bsr_anchor_codec_stream_bound(0) == 48 and lib.bsr_anchor_codec_stream_bound(1) == 48 + 8 + 2560
    assert lib.bsr_anchor_codec_stream_bound(257) == 48 + 12 + 2 * 2560
    assert lib.bsr_anchor_codec_stream_bound(-1) == 0 and lib.bsr_anchor_codec_stream_bound((1 << 27) + 1) == 0
    assert lib.bsr_anchor_codec_stream_bound(1 << 27) < 1 << 32
    assert lib.bsr_anchor_codec_scratch_bytes(0) == 256 and lib.bsr_anchor_codec_scratch_bytes(1 << 20) % 256 == 0
    assert lib.bsr_anchor_codec_scratch_bytes(1 << 20) >= 4 * (1 << 12) and lib.bsr_anchor_codec_scratch_bytes(-1) == 0
    assert (AC.MAGIC, AC.FORMAT, AC.HEADER_BYTES, AC.CHUNK, AC.ESCAPE) == (R.MAGIC, R.FORMAT, R.HEADER_BYTES, R.B, R.ESCAPE)
    assert struct.pack("<I", AC.MAGIC) == b"BSRA" and len(AC.STATUS) == 7


def test_native_calls_refuse_bad_arguments_before_any_launch():
    """Fake pointers only, never dereferenced on the host.  (The error string belongs to the calling thread: the calls are
    made on one that dies with it.)"""
    import threading
    lib = _capi.lib()
    P = 4096
    seen = []

    def refused(rc, word):
        seen.append((rc, word, _capi.last_error()))

    def calls():
        refused(lib.bsr_anchor_keys(-1, 0, None, 3, None, None, None, None, None, None), "N >= 0")
        refused(lib.bsr_anchor_keys(4, 5, P, 3, P, P, None, P, P, None), "n must be <= N")
        refused(lib.bsr_anchor_keys(4, 4, P, 2, P, P, None, P, P, None), "anchor_stride")
        refused(lib.bsr_anchor_keys(4, 4, P, 3, P, P, None, P + 4, P, None), "8-byte")
        refused(lib.bsr_anchor_keys(4, 4, P, 3, P, P, None, P, None, None), "NULL result")
        refused(lib.bsr_anchor_codec_encode(4, P, P, P, P, 10, P, P, None), "stream_bound")
        refused(lib.bsr_anchor_codec_encode(1 << 28, P, P, P, P, 10, P, P, None), "2^27")
        refused(lib.bsr_anchor_codec_encode(4, None, P, P, P, 1 << 20, P, P, None), "NULL keys")
        refused(lib.bsr_anchor_codec_decode(4, P + 2, 100, P, None, None, P, None), "4-byte")
        refused(lib.bsr_anchor_codec_decode(4, P, 100, None, None, None, P, None), "NULL anchor")

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert len(seen) == 10
    for rc, word, msg in seen:
        assert rc == 1 and word in msg and msg.startswith("bsr_anchor_"), (word, msg)


def test_python_checks_come_in_the_siblings_order():
    a, lo, hi = torch.zeros(5, 3), torch.zeros(3), torch.ones(1, 3)
    with pytest.raises(TypeError, match="_anchor must be float32"):      # a dtype before a shape and the device
        AC.encode_anchors(torch.zeros(5, 4, dtype=torch.float16), lo, hi)
    with pytest.raises(TypeError, match="bound_max must be a torch.Tensor"):
        AC.encode_anchors(a, lo, [1.0, 1.0, 1.0])
    with pytest.raises(TypeError, match="rows must be int64 or bool"):
        AC.encode_anchors(a, lo, hi, rows=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="3 dimensions"):
        AC.encode_anchors(torch.zeros(5, 3, 1), lo, hi)
    with pytest.raises(ValueError, match=r"_anchor must be \[N, 3\]"):
        AC.encode_anchors(torch.zeros(5, 4), lo, hi)
    with pytest.raises(ValueError, match="bound_min must hold 3 values"):
        AC.lattice_keys(a, torch.zeros(2), hi)
    with pytest.raises(ValueError, match="rows must be"):
        AC.encode_anchors(a, lo, hi, rows=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="_anchor must be on the GPU"):  # the device last
        AC.encode_anchors(a, lo, hi)
    with pytest.raises(TypeError, match="stream must be uint8"):
        AC.decode_anchors(torch.zeros(48, dtype=torch.int8))
    with pytest.raises(ValueError, match="one dimension"):
        AC.decode_anchors(torch.zeros(48, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="truncated"):
        AC.decode_anchors(torch.zeros(40, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a stream"):
        AC.decode_anchors(torch.zeros(48, dtype=torch.uint8))
    with pytest.raises(ValueError, match="device must be a GPU"):        # (refused before the stream is looked at)
        AC.decode_anchors(torch.zeros(48, dtype=torch.uint8), device="cpu")
    with pytest.raises(ValueError, match=r"n must be in \[0, 2\^27\]"):
        AC.decode_anchors(torch.zeros(48, dtype=torch.uint8), n=-1)
