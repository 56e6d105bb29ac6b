"""The entropy codec on the GPU (include/bloomscene_codec.h, bloomscene_amd/codec.py, torchac/) against the restatement
of tests/codec_reference.py: every stream BYTE-EQUAL to the restatement's, every decode bit-equal to the header's decoded
value ``float(rint(x / Q)) * Q`` (``rint(x / Q) * Q`` but for the sign of a zero).

Element counts are the smallest at which each mechanism can go wrong: 1, 63, 64, 65 (the lane boundary); 64 T - 1, 64 T,
64 T + 1 with the default T = 256 (the chunk boundary) and three chunks with a partial last one (the packing scan).  The
restatement's encoder costs milliseconds at these sizes; its decoder is not run here (tests/test_codec_cpu.py holds it
against the same expected values)."""
import numpy as np
import pytest
import torch

import codec_reference as R
import context_reference as CR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32


def _Cd():
    import bloomscene_amd.codec as Cd
    return Cd


def _d(a):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(DEV)


def _bytes(t):
    return t.cpu().numpy()


def _clean():
    """No deferred error is left behind, in the library or in the runtime."""
    from bloomscene_amd import _capi
    torch.cuda.synchronize()
    assert _capi.lib().bsr_check_deferred() == 0


def _both(x, mean, scale, Q, keep=None, r=1, T=256, scale_min=1e-9):
    """Encode and decode on the GPU; the stream against the restatement's, the decode against the expected values."""
    Cd = _Cd()
    Qd = float(Q) if np.asarray(Q).size == 1 and np.asarray(Q).ndim == 0 else _d(Q)
    stream = Cd.encode_gaussian(_d(x), _d(mean), _d(scale), Qd, keep=_d(keep), keep_repeat=r, scale_min=scale_min, T=T)
    ref = R.encode_gaussian(x, mean, scale, Q, keep=keep, keep_repeat=r, scale_min=scale_min, T=T)
    got = _bytes(stream)
    assert got.size == ref.size and (got == ref).all()
    y = Cd.decode_gaussian(stream, _d(mean), _d(scale), Qd, keep=_d(keep), keep_repeat=r, scale_min=scale_min).cpu().numpy()
    a, b = R.requantised(x, Q, keep, r)
    assert y.shape == x.shape and (y.view(np.uint32) == a.view(np.uint32)).all() and (y == b).all()
    return got


@pytest.mark.parametrize("n,C", [(1, 1), (9, 7), (8, 8), (5, 13), (127, 129), (256, 64), (5, 3277), (800, 50)])
def test_streams_are_the_restatements_at_the_lane_and_chunk_boundaries(n, C):
    assert n * C in (1, 63, 64, 65, 16383, 16384, 16385, 40000)
    x, mean, scale, Q = R.scene(n + C, n, C, 1.0, 0.25, "row")
    stream = _both(x, mean, scale, Q)
    h = R.parse(stream)
    assert h.chunks == (-(-n * C // 16384) if n * C > 1 else 0)          # (one element is one symbol: header only)
    if n * C == 40000:
        assert h.chunks == 3 and len(set(np.diff(h.offsets))) == 3     # three different sizes through the scan
    # a small T: many chunks, four to a workgroup, the last one partial
    if n * C in (65, 16385):
        assert R.parse(_both(x, mean, scale, Q, T=1)).chunks == -(-n * C // 64)


def test_strided_column_views_give_the_bytes_of_contiguous_copies():
    n, C = 300, 50
    x, mean, scale, Q = R.scene(11, n, C, 1.0, 0.25, "row")
    context = np.zeros((n, 175), f32)
    context[:, :C], context[:, C:2 * C] = mean, scale
    Cd = _Cd()
    cd = _d(context)
    xs = _d(np.concatenate([x, x], axis=1))[:, C:]
    views = Cd.encode_gaussian(xs, cd[:, :C], cd[:, C:2 * C], _d(Q)[:, 0])
    assert xs.stride(0) == 2 * C and cd[:, C:2 * C].stride(0) == 175
    dense = _both(x, mean, scale, Q)
    assert (_bytes(views) == dense).all()
    y = Cd.decode_gaussian(views, cd[:, :C], cd[:, C:2 * C], _d(Q))
    assert (y.cpu().numpy().view(np.uint32) == R.requantised(x, Q)[0].view(np.uint32)).all()


@pytest.mark.parametrize("q_shape", ["scalar", "row", "element"])
def test_step_sizes_as_one_value_per_row_and_per_element(q_shape):
    x, mean, scale, Q = R.scene(21, 70, 30, 0.5, 0.05, q_shape)
    _both(x, mean, scale, Q, T=8)


def test_keep_with_a_repeat_of_three():
    n, K = 90, 10
    x, mean, scale, Q = R.scene(31, n, 3 * K, 1.0, 0.05, "row")
    keep = (np.random.default_rng(31).random((n, K)) < 0.6).astype(f32)
    keep[7] = 0
    keep[n - 1] = 0
    stream = _both(x, mean, scale, Q, keep=keep, r=3, T=4)
    assert R.parse(stream).chunks == -(-n * 3 * K // 256)
    # a bool mask of BloomScene's shape [n, K, 1] is the same mask
    Cd = _Cd()
    again = Cd.encode_gaussian(_d(x), _d(mean), _d(scale), _d(Q), keep=_d(keep != 0).reshape(n, K, 1), keep_repeat=3, T=4)
    assert (_bytes(again) == stream).all()
    # nothing kept: a header-only stream and a zero decode
    none = np.zeros((n, K), f32)
    stream = _both(x, mean, scale, Q, keep=none, r=3)
    assert stream.size == R.HEADER_BYTES and R.parse(stream).L == 0
    # ... and no element at all
    empty = np.zeros((0, 30), f32)
    assert _both(empty, empty, empty, f32(0.25)).size == R.HEADER_BYTES


def test_one_two_and_the_most_symbols():
    # L == 1: header only
    one = np.full((70, 3), 0.26, f32)
    stream = _both(one, one * 0, one, f32(0.25))
    assert stream.size == R.HEADER_BYTES and (R.parse(stream).L, R.parse(stream).kmin) == (1, 1)
    # L == 2
    rng = np.random.default_rng(2)
    x = np.where(rng.random((40, 5)) < 0.3, 0.15, 0.2).astype(f32)
    stream = _both(x, np.full_like(x, 0.17), np.full_like(x, 0.03), f32(0.05))
    assert R.parse(stream).L == 2
    # L == 32767: two far-apart elements among near ones (15 trips of the bisection; the far ones have frequency 2)
    x, mean, scale, Q = R.scene(3, 30, 50, 1.0, 0.25)
    x[3, 4], x[20, 41] = -16383 * 0.25, 16383 * 0.25
    stream = _both(x, mean, scale, Q)
    h = R.parse(stream)
    assert (h.L, h.kmin) == (32767, -16383)
    # one more step is refused (below)


def test_point_mass_off_the_mean_and_the_forced_ends():
    x, mean, scale, Q = R.scene(4, 20, 10, 1.0, 0.25)
    scale[5] = 1e-9                       # a point-mass row ...
    x[5] = mean[5] + 1.0                  # ... whose symbols are four steps off the mean: frequency 2 each
    scale[6] = 0.0                        # below scale_min: clamped to it
    scale[7] = -1.0
    stream = _both(x, mean, scale, Q, T=2)
    h = R.parse(stream)
    model = R.gaussian_model(20, 10, mean, scale, Q, h.kmin, h.L)
    k, _ = R.symbols(x, np.full(200, Q, f32), 20, 10, np.ones(200, bool))
    j = k - h.kmin
    f = model.c(np.arange(200), j + 1) - model.c(np.arange(200), j)
    assert (f[50:60] == 2).all()
    assert (j == 0).any() and (j == h.L - 1).any()          # c(0) = 0 and c(L) = 65536, forced, are both in use
    # another scale_min is another model
    other = _both(x, mean, scale, Q, T=2, scale_min=0.5)
    assert other.size != stream.size or (other != stream).any()


def test_two_runs_give_identical_bytes():
    Cd = _Cd()
    x, mean, scale, Q = R.scene(5, 800, 50, 1.0, 0.25, "row")
    args = [_d(t) for t in (x, mean, scale, Q)]
    first = _bytes(Cd.encode_gaussian(*args))
    for _ in range(2):
        assert (_bytes(Cd.encode_gaussian(*args)) == first).all()


def test_decoding_shares_nothing_with_the_encoder_but_the_stream():
    """The operands of the decode are computed again, by a separate call, into other memory."""
    Cd = _Cd()
    s = CR.scene(200, 16, 32, 8, 4, seed=1)

    def operands():
        from bloomscene_amd import context as Cx
        context = Cx.context_head_maps(s.enc.to(DEV), [w.to(DEV) for w in s.weights], 8, 4)[0]
        return context[:, :8], context[:, 8:16]

    x = _d(R.scene(6, 200, 8, 1.0, 0.25)[0])
    mean, scale = operands()
    stream = Cd.encode_gaussian(x, mean, scale, 0.25)
    host = _bytes(stream).copy()
    del mean, scale, stream
    mean, scale = operands()
    y = Cd.decode_gaussian(_d(host), mean, scale, 0.25)
    assert (y.cpu().numpy().view(np.uint32) == R.requantised(x.cpu().numpy(), f32(0.25))[0].view(np.uint32)).all()
    ref = R.encode_gaussian(x.cpu().numpy(), mean.cpu().numpy(), scale.cpu().numpy(), f32(0.25))
    assert host.size == ref.size and (host == ref).all()


@pytest.mark.parametrize("p", [1e-6, 0.5, 1 - 1e-6])
def test_bernoulli_coder_with_one_row_for_all(p):
    Cd = _Cd()
    n = 16385
    sym = (np.random.default_rng(8).random(n) < p).astype(np.int16)
    sym[100] = 1 - sym[100]                     # (both symbols occur, whatever p)
    cdf = np.array([0, 1 - p, 1], f32)
    stream = Cd.encode_symbols(_d(sym), _d(cdf))
    ref = R.encode_table(sym, cdf)
    assert stream.numel() == ref.size and (_bytes(stream) == ref).all()
    assert (Cd.decode_symbols(stream, _d(cdf), n).cpu().numpy() == sym).all()
    # the same table as a row per symbol: the same bytes
    rows = Cd.encode_symbols(_d(sym), _d(np.tile(cdf, (n, 1))))
    assert (_bytes(rows) == ref).all()


def test_table_of_rows_round_trips_through_the_torchac_shim_from_cpu_tensors():
    import torchac
    rng = np.random.default_rng(9)
    n, L = 700, 37
    steps = np.sort(rng.random((n, L - 1)), axis=1).astype(f32)
    cdf = np.concatenate([np.zeros((n, 1), f32), steps, np.ones((n, 1), f32)], axis=1)
    sym = rng.integers(0, L, n).astype(np.int16)
    data = torchac.encode_float_cdf(torch.from_numpy(cdf), torch.from_numpy(sym), check_input_bounds=True)
    assert isinstance(data, bytes)
    ref = R.encode_table(sym, cdf)
    assert len(data) == ref.size and (np.frombuffer(data, np.uint8) == ref).all()
    out = torchac.decode_float_cdf(torch.from_numpy(cdf), data)
    assert out.dtype == torch.int16 and out.device.type == "cpu" and (out.numpy() == sym).all()
    out = torchac.decode_float_cdf(_d(cdf).reshape(7, 100, L + 1), data)
    assert out.device.type == "cuda" and tuple(out.shape) == (7, 100) and (out.cpu().numpy().reshape(-1) == sym).all()


def test_refusals_raise_and_leave_nothing_behind():
    Cd = _Cd()
    x, mean, scale, Q = R.scene(9, 300, 60, 1.0, 0.25)
    good = [_d(t) for t in (x, mean, scale)]

    def encode(x=good[0], mean=good[1], scale=good[2], Q=0.25):
        return Cd.encode_gaussian(x, mean, scale, Q)

    xb = good[0].clone()
    xb[100, 7] = float("nan")
    with pytest.raises(ValueError, match="non-finite x / Q"):
        encode(x=xb)
    _clean()
    with pytest.raises(ValueError, match="Q <= 0"):
        encode(Q=0.0)
    _clean()
    with pytest.raises(ValueError, match="Q <= 0"):
        encode(Q=torch.full((300, 1), float("inf"), device=DEV))
    mb = good[1].clone()
    mb[299, 59] = float("-inf")
    with pytest.raises(ValueError, match="non-finite mean or scale"):
        encode(mean=mb)
    _clean()
    xb = good[0].clone()
    xb[0, 0], xb[299, 59] = -16383 * 0.25, 16384 * 0.25              # 32768 symbols
    with pytest.raises(ValueError, match="more than 32767 symbols"):
        encode(x=xb)
    _clean()
    # the decoder's
    stream = encode()
    assert (_bytes(stream) == R.encode_gaussian(x, mean, scale, Q)).all()
    wrong = stream.clone()
    wrong[0] ^= 1
    with pytest.raises(ValueError, match="not a stream of this codec"):
        Cd.decode_gaussian(wrong, good[1], good[2], 0.25)
    _clean()
    with pytest.raises(ValueError, match="not a stream of this codec"):
        Cd.decode_gaussian(stream, good[1][:299], good[2][:299], 0.25)              # another element count
    # a truncated stream, as a prefix VIEW of the full, larger allocation: the guard's answer is checked without
    # depending on the guard for memory safety
    for cut in (2, 300, stream.numel() - 40, stream.numel() - 8):
        with pytest.raises(ValueError, match="truncated"):
            Cd.decode_gaussian(stream[:stream.numel() - cut], good[1], good[2], 0.25)
        _clean()
    # a flipped word: the lanes do not return to their start state (or run out of words)
    corrupt = stream.clone()
    corrupt[-3] ^= 0x55
    with pytest.raises(ValueError, match="corrupt|truncated"):
        Cd.decode_gaussian(corrupt, good[1], good[2], 0.25)
    _clean()
    # the table model
    cdf = np.tile(np.array([0, 0.3, 0.6, 1], f32), (500, 1))
    sym = _d(np.random.default_rng(1).integers(0, 3, 500).astype(np.int16))
    table = Cd.encode_symbols(sym, _d(cdf))
    cdf[317] = [0, 0.6, 0.3, 1]
    with pytest.raises(ValueError, match="not non-decreasing"):
        Cd.encode_symbols(sym, _d(cdf))
    _clean()
    with pytest.raises(ValueError, match="not non-decreasing"):
        Cd.decode_symbols(table, _d(cdf), 500)
    cdf[317] = [0, 0.3, 0.6, 1]
    symb = sym.clone()
    symb[499] = 3
    with pytest.raises(ValueError, match="symbol outside"):
        Cd.encode_symbols(symb, _d(cdf))
    with pytest.raises(ValueError, match="not a stream of this codec"):
        Cd.decode_gaussian(table, good[1], good[2], 0.25)                           # the other model's stream
    _clean()
    # and the good calls still give what they gave
    assert (_bytes(encode()) == _bytes(stream)).all()
    assert (Cd.decode_symbols(table, _d(cdf), 500) == sym).all()


def test_drop_ins_round_trip_through_files(tmp_path):
    Cd = _Cd()
    x, mean, scale, Q = R.scene(12, 1, 4099, 1.0, 0.25, "element")
    xd, md, sd, Qd = (_d(t.reshape(-1)) for t in (x, mean, scale, Q))
    name = str(tmp_path / "feat.b")
    bits, lo, hi = Cd.encoder_gaussian(xd, md, sd, Qd, file_name=name)
    data = np.fromfile(name, np.uint8)
    ref = R.encode_gaussian(x, mean, scale, Q)
    assert bits == 8 * data.size and data.size == ref.size and (data == ref).all()
    k = np.rint(x / Q)
    assert (float(lo), float(hi)) == (float(k.min()), float(k.max()))
    y = Cd.decoder_gaussian(md, sd, Qd, file_name=name, min_value=lo, max_value=hi)
    assert tuple(y.shape) == (4099,) and (y.cpu().numpy().view(np.uint32) == R.requantised(x, Q)[0].reshape(-1).view(np.uint32)).all()
    # a number for Q, as the reference allows
    bits, lo, hi = Cd.encoder_gaussian(xd, md, sd, 0.25, file_name=name)
    assert (Cd.decoder_gaussian(md, sd, 0.25, file_name=name).cpu().numpy() == R.requantised(x, f32(0.25))[1].reshape(-1)).all()
    # the Bernoulli pair: x in {-1, +1}, p per element (the reference fills a tensor with one value)
    rng = np.random.default_rng(13)
    signs = np.where(rng.random(5000) < 0.2, 1.0, -1.0).astype(f32)
    p = torch.full((5000,), float((signs > 0).mean()))
    name = str(tmp_path / "masks.b")
    bits = Cd.encoder(_d(signs), p.to(DEV), name)
    data = np.fromfile(name, np.uint8)
    cdf = np.array([0, 1 - f32(p[0].item()), 1], f32)
    ref = R.encode_table(((signs + 1) / 2).astype(np.int16), np.tile(cdf, (5000, 1)))
    assert bits == 8 * data.size and data.size == ref.size and (data == ref).all()
    out = Cd.decoder(p.to(DEV), name)
    assert out.dtype == torch.float32 and out.device.type == "cuda" and (out.cpu().numpy() == signs).all()
    assert (Cd.decoder(p, name).numpy() == signs).all()               # a CPU p: the result comes back to the CPU


def test_whole_model_streams_reproduce_the_quantiser():
    """encode_attributes / decode_attributes from the outputs of context_head_maps and context_quantise(steps=True), all
    anchors at once; 333 anchors: no multiple of 64."""
    from bloomscene_amd import context as Cx
    Cd = _Cd()
    F, K, n = 8, 4, 333
    s = CR.scene(n, 16, 32, F, K, seed=3)
    enc, weights = s.enc.to(DEV), [w.to(DEV) for w in s.weights]
    # (a quarter of the synthetic scaling: as drawn it spans 36 000 steps of its Q, beyond the reference's int16 range too)
    feat, gs, go = s.feat.to(DEV), (s.grid_scaling * 0.25).to(DEV), s.grid_offsets.to(DEV)
    means = [feat.mean(), gs.mean(), go.mean()]
    feat_q, gs_q, go_q, Q = Cx.context_quantise_tensors(enc, weights, F, K, feat, gs, go, *means, steps=True)
    context = Cx.context_head_maps(enc, weights, F, K)[0]
    masks = (torch.rand(n, K, 1, generator=torch.Generator().manual_seed(3)) < 0.7).float().to(DEV)
    masks[5] = 0
    streams = Cd.encode_attributes(context, Q, feat_q, gs_q, go_q, masks, F, K)
    assert len(streams) == 3 and all(t.dtype == torch.uint8 and t.device.type == "cuda" for t in streams)
    out = Cd.decode_attributes(streams, context, Q, masks, F, K)
    cn, Qn = context.cpu().numpy(), Q.cpu().numpy()
    blocks = ((0, F, F), (2 * F, 6, 6), (2 * F + 12, 3 * K, 3 * K))
    keeps = (None, None, masks.cpu().numpy().reshape(n, K))
    for c, (got, x, (at, C, gap), keep) in enumerate(zip(out, (feat_q, gs_q, go_q), blocks, keeps)):
        xn = x.cpu().numpy().reshape(n, C)
        a, b = R.requantised(xn, Qn[:, c:c + 1], keep, 3 if keep is not None else 1)
        assert tuple(got.shape) == tuple(x.shape)
        assert (got.cpu().numpy().reshape(n, C).view(np.uint32) == a.view(np.uint32)).all()
        ref = R.encode_gaussian(xn, cn[:, at:at + C], cn[:, at + gap:at + gap + C], Qn[:, c:c + 1], keep=keep,
                                keep_repeat=3 if keep is not None else 1)
        assert streams[c].numel() == ref.size and (_bytes(streams[c]) == ref).all()
