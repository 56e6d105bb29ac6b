"""GPU tests of the anchor position coder (include/bloomscene_anchor_codec.h, bloomscene_amd/anchor_codec.py): the kernels'
stream is BYTE-EQUAL to the restatement's (tests/anchor_codec_reference.py) and the decoder's anchors are BIT-EQUAL to
anchor_state.visible's in permuted order, at every chunk edge and on the key patterns that take the coder's other paths;
the permutation is the stable argsort of the keys; two runs agree; every refusal is raised by name."""
import struct

import numpy as np
import pytest
import torch

import anchor_codec_reference as R
from bloomscene_amd import _capi
from bloomscene_amd import anchor_codec as AC
from bloomscene_amd import anchor_state as AS
from bloomscene_amd._operands import ptr

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
BMIN, BMAX = np.array([-1.5, -0.75, 0.25], f32), np.array([2.5, 1.25, 3.0], f32)
TOP = (1 << 48) - 1


def from_keys(keys):
    """Anchors in the middle of the lattice cells of ``keys`` (float64, then one rounding): their keys are ``keys``."""
    keys = np.asarray(keys, np.uint64)
    q = np.stack([(keys >> np.uint64(s)) & np.uint64(0xffff) for s in (32, 16, 0)], axis=1).astype(np.float64)
    interval = R.interval_np(BMIN, BMAX).astype(np.float64)
    return ((q + 0.5) * interval + BMIN.astype(np.float64)).astype(f32)


def random_anchors(n, seed, lo=-0.1, hi=1.1):
    rng = np.random.default_rng(seed)
    return (BMIN + (BMAX - BMIN) * rng.uniform(lo, hi, (n, 3))).astype(f32)


def cases():
    rng = np.random.default_rng(21)
    out = {f"n = {n}": (random_anchors(n, n), None) for n in (0, 1, 2, 255, 256, 257, 513)}
    out["all keys equal (mean == 0)"] = (from_keys([0x123456789abc] * 300), None)
    dup = np.repeat(rng.integers(0, 1 << 48, 90, dtype=np.uint64), 6)            # 540 keys: runs of 6 cross 256 and 512
    out["duplicates inside and across a chunk edge"] = (from_keys(rng.permutation(dup)), None)
    near = rng.integers(0, 1 << 18, 128, dtype=np.uint64)
    out["two far-apart clusters in a chunk (the escape)"] = (from_keys(np.concatenate([near, near + np.uint64(1 << 46)])), None)
    out["keys 0 and 2^48 - 1 (k = 47)"] = (from_keys([TOP, 0]), None)
    out["clamped at 0 and at 65535"] = (random_anchors(400, 5, -2.0, 3.0), None)
    out["a row-strided view"] = (random_anchors(300, 6), "strided")
    out["rows as a list"] = (random_anchors(600, 7), np.sort(rng.choice(600, 300, replace=False)).astype(np.int64))
    shuffled = rng.permutation(600)[:300].astype(np.int64)
    dup_rows = random_anchors(600, 9)
    dup_rows[shuffled[:100]] = dup_rows[shuffled[100:200]]                        # equal keys at rows listed out of order
    out["rows as an unsorted list (ties by source row)"] = (dup_rows, shuffled)
    out["rows as a mask"] = (random_anchors(600, 8), rng.random(600) < 0.5)
    return out


CASES = cases()


def device_anchor(anchor, how):
    if isinstance(how, str):                                                  # rows of a wider tensor, read in place
        wide = torch.zeros(anchor.shape[0], 7, dtype=torch.float32, device=DEV)
        wide[:, 2:5] = torch.from_numpy(anchor).to(DEV)
        view = wide[:, 2:5]
        assert not view.is_contiguous()
        return view
    return torch.from_numpy(anchor).to(DEV)


def visible_anchors(anchor_t, lo, hi):
    """get_anchor of every row through the training path's kernel (bsr_anchor_visible_forward)."""
    N = anchor_t.shape[0]
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    return AS.visible(torch.arange(N, device=DEV), anchor_t.contiguous(), lo, hi, z(N, 1), z(N, 1, 3), z(N, 6), z(N, 1, 1))[0]


@pytest.mark.parametrize("name", list(CASES))
def test_stream_is_the_restatements_and_decodes_to_the_visible_anchors(name):
    anchor, how = CASES[name]
    rows = None if how is None or isinstance(how, str) else how
    want_stream, want_perm = R.encode_np(anchor, BMIN, BMAX, rows)
    want_keys = R.keys_np(anchor, BMIN, BMAX)
    if name.startswith("keys 0 and"):
        assert sorted(want_keys.tolist()) == [0, TOP]
    if name.startswith("clamped"):
        fields = np.stack([(want_keys >> np.uint64(s)) & np.uint64(0xffff) for s in (32, 16, 0)], axis=1)
        assert (fields == 0).any() and (fields == 65535).any()
    if "escape" in name:
        ks = np.sort(want_keys).astype(object)
        assert max(int(d) for d in np.diff(ks)) >> R.rice_k(int(ks[0]), int(ks[-1]), ks.size) >= R.ESCAPE and ks.size == 256
    a = device_anchor(anchor, how)
    lo, hi = torch.from_numpy(BMIN).to(DEV), torch.from_numpy(BMAX).reshape(1, 3).to(DEV)
    r = None if rows is None else torch.from_numpy(rows).to(DEV)
    stream, perm = AC.encode_anchors(a, lo, hi, rows=r)
    assert stream.dtype == torch.uint8 and bytes(stream.cpu().numpy()) == want_stream
    assert perm.dtype == torch.int64 and (perm.cpu().numpy() == want_perm).all()
    # perm is the stable argsort of the keys
    keys = AC.lattice_keys(a, lo, hi, rows=r)
    picked = want_keys if rows is None else want_keys[np.nonzero(rows)[0] if rows.dtype == np.bool_ else rows]
    assert (keys.cpu().numpy().astype(np.uint64) == picked).all()
    listed = np.arange(anchor.shape[0]) if rows is None else (np.nonzero(rows)[0] if rows.dtype == np.bool_ else rows)
    by_key_then_row = listed[np.lexsort((listed, picked))]                       # the stable argsort of (key, source row)
    assert (perm.cpu().numpy() == by_key_then_row).all()
    if name.startswith("rows as an unsorted"):
        same = np.diff(picked[np.lexsort((listed, picked))].astype(np.int64)) == 0
        assert same.sum() >= 100 and (np.diff(by_key_then_row)[same] > 0).all()
    # the decoder: from the stream alone, and with n given
    n = want_perm.size
    got, dlo, dhi, dkeys = AC.decode_anchors(stream, return_keys=True)
    assert got.shape == (n, 3) and (dlo.cpu().numpy() == BMIN).all() and (dhi.cpu().numpy() == BMAX).all()
    assert (dkeys.cpu().numpy().astype(np.uint64) == want_keys[want_perm]).all()
    assert (got.cpu().numpy().view(np.uint32) == R.dequantise_np(want_keys[want_perm], BMIN, BMAX).view(np.uint32)).all()
    if anchor.shape[0]:
        vis = visible_anchors(a, lo, hi)[perm]
        assert torch.equal(got.view(torch.int32), vis.view(torch.int32))
    again = AC.decode_anchors(stream.cpu(), n=n, device=DEV)[0]
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    # bit-identical from run to run
    stream2, perm2 = AC.encode_anchors(a, lo, hi, rows=r)
    assert torch.equal(stream, stream2) and torch.equal(perm, perm2)


def encoded(keys):
    a = torch.from_numpy(from_keys(keys)).to(DEV)
    stream, _ = AC.encode_anchors(a, torch.from_numpy(BMIN).to(DEV), torch.from_numpy(BMAX).to(DEV))
    assert bytes(stream.cpu().numpy()) == R.encode_keys(sorted(int(k) for k in keys), BMIN, BMAX)
    return stream.clone()


def test_each_refusal_is_raised_by_name():
    lo, hi = torch.from_numpy(BMIN).to(DEV), torch.from_numpy(BMAX).to(DEV)
    bad = random_anchors(300, 1)
    bad[77, 1] = np.nan
    with pytest.raises(ValueError, match="encode_anchors: a non-finite coordinate"):
        AC.encode_anchors(torch.from_numpy(bad).to(DEV), lo, hi)
    bad[77, 1] = np.inf
    with pytest.raises(ValueError, match="lattice_keys: a non-finite coordinate"):
        AC.lattice_keys(torch.from_numpy(bad).to(DEV), lo, hi)
    with pytest.raises(ValueError, match="a non-finite coordinate"):
        AC.encode_anchors(torch.from_numpy(random_anchors(10, 1)).to(DEV), lo, hi * float("inf"))
    with pytest.raises(ValueError, match=r"a row outside \[0, N\)"):
        AC.encode_anchors(torch.from_numpy(random_anchors(10, 1)).to(DEV), lo, hi, rows=torch.tensor([1, 10], device=DEV))

    keys = np.sort(np.random.default_rng(5).integers(0, 1 << 30, 600)).astype(np.uint64)
    stream = encoded(keys)
    n, table = 600, 48 + 4 * 4
    for cut, what in ((20, "truncated"), (48 + 6, "truncated"), (table + 100, "truncated")):
        with pytest.raises(ValueError, match="decode_anchors: a " + what):        # the kernel's finding (n is given)
            AC.decode_anchors(stream[:cut], n=n)
    with pytest.raises(ValueError, match="truncated"):                            # the host's, from the header
        AC.decode_anchors(stream[:20])
    with pytest.raises(ValueError, match="not a stream of this coder"):
        AC.decode_anchors(stream, n=n + 1)
    host = stream.cpu().numpy().copy()
    swapped = host.copy()
    swapped[52:56], swapped[56:60] = host[56:60], host[52:56]
    with pytest.raises(ValueError, match="a corrupt stream"):
        AC.decode_anchors(torch.from_numpy(swapped).to(DEV))
    for at, value in ((0, 0), (4, 2), (16, 128), (20, 16), (12, 2)):
        wrong = host.copy()
        wrong[at:at + 4] = np.frombuffer(struct.pack("<I", value), np.uint8)
        with pytest.raises(ValueError, match="not a stream of this coder"):
            AC.decode_anchors(torch.from_numpy(wrong).to(DEV), n=n)
    # one flipped byte in a chunk's bits.  All gaps 0 (k = 0, one zero bit each): the flipped byte is one gap of 8 in 9 bits
    # where 8 gaps took 8, so the chunk's 255 gaps need 263 bits of its 256: a code runs past the chunk's end.  (The format
    # has no checksum: a flip inside a gap's low bits decodes to other keys, include/bloomscene_anchor_codec.h.)
    flat = encoded([0x5555] * 256)
    assert flat.numel() == 48 + 8 + 8 + 32
    flat[48 + 8 + 8 + 5] ^= 0xff
    with pytest.raises(ValueError, match="a corrupt stream"):
        AC.decode_anchors(flat)
    # bits that no code uses, and padding that is not zero
    loose = encoded([7] * 200)                                                   # 199 bits in 7 words
    loose[48 + 8 + 8 + 27] |= 0x80
    with pytest.raises(ValueError, match="a corrupt stream"):
        AC.decode_anchors(loose)
    # a gap that takes a key beyond 48 bits
    high = encoded([TOP - 5, TOP - 1])                                           # k = 2: '10' + 00; make it 4 * 2 + ... -> '110'
    assert high[48 + 8 + 8] == 0b0001
    high[48 + 8 + 8] = 0b0011
    with pytest.raises(ValueError, match="2\\^48"):
        AC.decode_anchors(high)


def test_the_encoder_refuses_unsorted_and_wide_keys():
    lib = _capi.lib()
    bound = torch.from_numpy(np.concatenate([BMIN, BMAX])).to(DEV)
    for keys, what in (([3, 2, 5], 4), ([1, 1 << 48], 8), (list(range(255, -1, -1)) + [300], 4)):
        k = torch.tensor(keys, dtype=torch.int64, device=DEV)
        n = k.numel()
        stream = torch.zeros(lib.bsr_anchor_codec_stream_bound(n), dtype=torch.uint8, device=DEV)
        scratch = torch.zeros(lib.bsr_anchor_codec_scratch_bytes(n), dtype=torch.uint8, device=DEV)
        result = torch.zeros(2, dtype=torch.int32, device=DEV)
        _capi.call("bsr_anchor_codec_encode", n, ptr(k), ptr(bound), ptr(bound[3:]), ptr(stream), stream.numel(), ptr(result),
                   ptr(scratch), torch.cuda.current_stream().cuda_stream)
        assert result.tolist() == [what, 0]
