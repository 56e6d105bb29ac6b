"""CPU tests of the anchor state (include/bloomscene_anchor_state.h, bloomscene_amd/anchor_state.py): the restatements of
tests/anchor_state_reference.py against torch's own operations, the library's entry points, and the python interface's
checks -- all before the device is touched."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import anchor_state_reference as AR
from bloomscene_amd import _capi
from bloomscene_amd import anchor_state as AS

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def test_floor_division_restatement_is_torchs_bit_for_bit():
    rng = np.random.default_rng(3)
    bmin = np.array([-1.5, -0.75, 0.25], f32)
    bmax = np.array([2.5, 1.25, 3.0], f32)
    interval = ((bmax - bmin) * f32(AR.Q_ANCHOR)).astype(f32) + f32(1e-6)
    q = np.concatenate([np.arange(0, 65536, 7), [65535]]).astype(f32)
    exact = ((q[:, None] * interval).astype(f32) + bmin).astype(f32)                  # exact multiples q * interval + min
    spread = (bmin + (bmax - bmin) * rng.uniform(-0.25, 1.25, (20000, 3))).astype(f32)  # below min and above max as well
    anchors = np.concatenate([exact, spread, bmin[None], bmax[None], np.nextafter(exact[:500], f32(np.inf)),
                              np.nextafter(exact[:500], f32(-np.inf))])
    a = (anchors - bmin).astype(f32)
    b = np.broadcast_to(interval, a.shape)
    ref = torch.div(torch.from_numpy(a), torch.from_numpy(b.copy()), rounding_mode="floor").numpy()
    got = AR.floor_div_np(a, b)
    assert (_bits(got) == _bits(ref)).all()
    assert (ref < 0).any() and (ref > 65535).any()                                    # the clamp has work to do
    assert (got != np.floor((a / b).astype(f32))).any()                               # (and it is not floorf(a / b))
    # signs of both operands, zeros and a zero divisor
    a2 = (rng.standard_normal(20000) * 10.0 ** rng.uniform(-3, 3, 20000)).astype(f32)
    b2 = (rng.standard_normal(20000) * 10.0 ** rng.uniform(-3, 3, 20000)).astype(f32)
    a2[:50], b2[50:60] = 0, 0
    a2[100:200] = (np.rint(a2[100:200]) * b2[100:200]).astype(f32)
    ref2 = torch.div(torch.from_numpy(a2), torch.from_numpy(b2), rounding_mode="floor").numpy()
    assert (_bits(AR.floor_div_np(a2, b2)) == _bits(ref2)).all()


@pytest.mark.parametrize("degenerate", (False, True))
def test_quantised_anchor_is_the_eager_lines(degenerate):
    s = AR.scene(400, 4, 2, 400, seed=5)
    bmax = s.bmin.copy() if degenerate else s.bmax                                    # max == min: the 1e-6 interval alone
    got = AR.quantize_anchor_np(s.anchor, s.bmin, bmax)
    t = torch.from_numpy
    ref = AR._QuantizeAnchor.apply(t(s.anchor), t(s.bmin)[None], t(bmax)[None]).numpy()
    assert (_bits(got) == _bits(ref)).all()
    assert (got == s.bmin).any() and (degenerate or (got != s.bmin).any())


def test_visible_restatement_against_the_eager_lines_on_cpu():
    s = AR.scene(129, 5, 3, 65)
    t = torch.from_numpy
    got = AR.visible_np(s.idx, s.anchor, s.bmin, s.bmax, s.feat, s.offset, s.scaling, s.mask)
    ref = AR.eager_visible(t(s.idx), t(s.anchor), t(s.bmin)[None], t(s.bmax)[None], t(s.feat), t(s.offset), t(s.scaling), t(s.mask))
    for i in (0, 1, 2):
        assert (_bits(got[i]) == _bits(ref[i].numpy())).all(), i
    assert np.array_equal(got[4] > 0.5, ref[4].numpy() > 0.5) and set(np.unique(got[4])) == {0.0, 1.0}
    assert np.array_equal(got[5], ref[5].numpy()) and 0 < got[5].sum() < 65     # some anchors have all K zero
    assert got[6] == ref[6].numpy()
    assert np.abs(got[3].astype(np.float64) / np.exp(s.scaling[s.idx].astype(np.float64)) - 1).max() < 1.01 * 2.0 ** -23
    # an index out of range gives a zero row and counts for nothing
    bad = s.idx.copy()
    bad[3], bad[7] = -1, 129
    out = AR.visible_np(bad, s.anchor, s.bmin, s.bmax, s.feat, s.offset, s.scaling, s.mask)
    for o in out[:5]:
        assert not o[3].any() and not o[7].any()
    assert not out[5][3] and not out[5][7]


@pytest.mark.parametrize("case", ("plain", "short", "padded", "bool"))
def test_accumulate_restatement_is_the_eager_lines(case):
    N, K, n = 300, 10, 290
    kw = dict(plain={}, short=dict(M=900), padded=dict(padded=57), bool=dict(bool_filter=True))[case]
    s = AR.epilogue_scene(N, K, n, integer_norms=True, blocks=("none", "all", "mixed"), **kw)
    got = AR.accumulate_np(s.acc, s.idx, s.opacity, s.selection, s.radii, s.grad, K)
    t = torch.from_numpy
    if case == "short":       # the eager lines need one row per selected candidate: pad with radius 0 (never a target)
        radii = np.concatenate([s.radii, np.zeros(s.count - s.M, np.int32)])
        grad = np.concatenate([s.grad, np.ones((s.count - s.M, 3), f32)])
    else:                     # ... and exactly one: the padded form's extra rows are cut off
        radii, grad = s.radii[:s.count], s.grad[:s.count]
    keep = t(radii) if radii.dtype == np.bool_ else t(radii) > 0
    ref = AR.eager_accumulate([t(a) for a in s.acc], t(s.idx), t(s.opacity), t(s.selection), keep, t(grad), K)
    for i in (1, 2, 3):       # integer-valued: the norms are those of Pythagorean triples
        assert torch.equal(t(got[i]).view(-1, 1), ref[i]), i
    assert (got[2] != s.acc[2].reshape(-1)).any() and (got[3] != s.acc[3].reshape(-1)).any()
    bound = (K - 1) * 2.0 ** -24 * np.abs(s.opacity.astype(np.float64)).reshape(n, K).sum(axis=1)
    full = np.zeros(N)
    full[s.idx] = bound
    err = np.abs(got[0].astype(np.float64) - ref[0].numpy().reshape(-1).astype(np.float64))
    assert (err <= full + 2.0 ** -24 * np.abs(ref[0].numpy().reshape(-1))).all()      # (+ the rounding of the final +=)
    untouched = np.setdiff1d(np.arange(N), s.idx)
    assert (got[0][untouched] == s.acc[0].reshape(-1)[untouched]).all() and (got[1][untouched] == s.acc[1].reshape(-1)[untouched]).all()
    if case == "short":       # the selected candidates beyond M are untouched
        c = np.nonzero(s.selection)[0][s.M:]
        target = s.idx[c // K] * K + c % K
        assert (got[2][target] == s.acc[2].reshape(-1)[target]).all() and (got[3][target] == s.acc[3].reshape(-1)[target]).all()


def test_entry_points_exist_and_size_their_scratch():
    lib = _capi.lib()
    for name in ("bsr_anchor_visible_forward", "bsr_anchor_visible_backward", "bsr_anchor_accumulate_scratch_bytes",
                 "bsr_anchor_accumulate"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert lib.bsr_version() == 4
    size = lib.bsr_anchor_accumulate_scratch_bytes
    for n, K in ((0, 10), (-1, 10), (10, 0), (10, 17), (2 ** 31 // 30 + 1, 10)):
        assert size(n, K) == 0, (n, K)
    sizes = [size(n, 10) for n in (1, 100, 1000, 10000, 100000, 1000000)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0] and all(s % 256 == 0 for s in sizes)
    assert size(100000, 10) >= 4 * -(-100000 * 10 // AS.SCAN_BLOCK)                    # one count per scan block
    assert AS.SCAN_BLOCK == AR.SCAN_BLOCK


def test_c_entry_points_name_the_argument_they_refuse():
    lib = _capi.lib()
    seen = []
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)

    def forward(N, n, F, K, fs=64, p=None, rate=None):
        return lib.bsr_anchor_visible_forward(N, n, F, K, p, p, p, p, p, fs, p, p, p, p, p, p, p, p, p, rate, None)

    def backward(N, n, F, K, p=None):
        return lib.bsr_anchor_visible_backward(N, n, F, K, None, p, p, p, p, p, p, p, addr, p, p, p, p, None)

    def accumulate(N, n, K, M, p=None, scratch=None):
        return lib.bsr_anchor_accumulate(N, n, K, M, p, p, p, p, 0, p, p, p, p, p, scratch, None)

    def calls():             # (the error string belongs to the calling thread: this one's dies with it)
        for N, n, F, K, word in ((-1, 0, 4, 1, "N must"), (4, 5, 4, 1, "n must"), (4, -1, 4, 1, "n must"), (4, 1, 0, 1, "F must"),
                                 (4, 1, 65, 1, "F must"), (4, 1, 4, 0, "K must"), (4, 1, 4, 17, "K must"),
                                 (2 ** 31 // 64 + 1, 1, 64, 1, "2^31"), (2 ** 31 // 48 + 1, 1, 4, 16, "2^31")):
            seen.append((forward(N, n, F, K), word in _capi.last_error()))
            seen.append((backward(N, n, F, K), word in _capi.last_error()))
        seen.append((forward(4, 1, 4, 1, fs=3), "feat_stride" in _capi.last_error()))
        seen.append((forward(4, 0, 4, 1), "NULL out_rate" in _capi.last_error()))
        seen.append((forward(4, 1, 4, 1, rate=addr), "NULL idx" in _capi.last_error()))
        seen.append((forward(4, 1, 4, 1, p=addr + 2, rate=addr), "out_mask_anchor must be 4-byte aligned" in _capi.last_error()))
        seen.append((backward(4, 1, 4, 1), "NULL idx" in _capi.last_error()))
        seen.append((accumulate(4, 5, 1, 0), "n must" in _capi.last_error()))
        seen.append((accumulate(4, 1, 17, 0), "K must" in _capi.last_error()))
        seen.append((accumulate(4, 1, 1, -1), "M must" in _capi.last_error()))
        seen.append((accumulate(4, 1, 1, 0), "NULL idx" in _capi.last_error()))
        seen.append((accumulate(4, 1, 1, 0, p=addr), "NULL scratch" in _capi.last_error()))
        seen.append((1 - accumulate(4, 0, 1, 0), True))                                # n == 0 launches nothing
        seen.append((1 - lib.bsr_anchor_visible_backward(4, 0, 4, 1, *([None] * 14)), True))  # no gradient asked for

    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert seen == [(1, True)] * len(seen), seen


def test_python_checks_come_before_the_device_in_the_siblings_order():
    s = AR.scene(12, 6, 2, 5)
    t = torch.from_numpy
    ok = dict(idx=t(s.idx), _anchor=t(s.anchor), x_bound_min=t(s.bmin)[None], x_bound_max=t(s.bmax)[None], _anchor_feat=t(s.feat),
              _offset=t(s.offset), _scaling=t(s.scaling), _mask=t(s.mask))

    def call(**kw):
        return AS.visible(**{**ok, **kw})

    # a wrong dtype first, even with a wrong shape and a bound that wants a gradient beside it
    with pytest.raises(TypeError, match="_anchor must be float32"):
        call(_anchor=t(s.anchor).double()[:, :2], x_bound_min=t(s.bmin).requires_grad_(True))
    with pytest.raises(TypeError, match="idx must be int64"):
        call(idx=t(s.idx).int())
    with pytest.raises(TypeError, match="_mask must be a torch.Tensor"):
        call(_mask=s.mask)
    # then what is not implemented, before any shape
    with pytest.raises(NotImplementedError, match="x_bound_min requires a gradient"):
        call(x_bound_min=t(s.bmin).requires_grad_(True), _scaling=t(s.scaling)[:, :5])
    # then shapes
    with pytest.raises(ValueError, match=r"_scaling must be \[12, 6\]"):
        call(_scaling=t(s.scaling)[:, :5])
    with pytest.raises(ValueError, match=r"_offset must be \[12, K, 3\]"):
        call(_offset=t(s.offset)[:11])
    with pytest.raises(ValueError, match="F = _anchor_feat.shape"):
        call(_anchor_feat=torch.zeros(12, 65))
    with pytest.raises(ValueError, match="K = _offset.shape"):
        call(_offset=torch.zeros(12, 17, 3))
    with pytest.raises(ValueError, match="x_bound_max must hold 3"):
        call(x_bound_max=torch.zeros(4))
    with pytest.raises(ValueError, match="more than the 12 anchors"):
        call(idx=torch.arange(13))
    with pytest.raises(ValueError, match=r"idx must be \[n\]"):
        call(idx=t(s.idx)[None])
    # and the device last: everything else is right, there is no CPU path
    with pytest.raises(ValueError, match="idx must be on the GPU"):
        call()
    with pytest.raises(ValueError, match="on the GPU"):
        call(_mask=t(s.mask)[:, :, 0], x_bound_min=t(s.bmin), check=True)

    e = AR.epilogue_scene(12, 2, 5)
    oke = dict(opacity_accum=t(e.acc[0]), anchor_demon=t(e.acc[1]), offset_gradient_accum=t(e.acc[2]), offset_denom=t(e.acc[3]),
               idx=t(e.idx), neural_opacity=t(e.opacity), offset_selection_mask=t(e.selection), radii=t(e.radii),
               viewspace_grad=t(e.grad))

    def acc(**kw):
        return AS.accumulate(**{**oke, **kw})

    with pytest.raises(ValueError, match="viewspace_grad is None"):
        acc(viewspace_grad=None, radii=t(e.radii).long())
    with pytest.raises(TypeError, match="radii must be int32 or bool"):
        acc(radii=t(e.radii).long(), anchor_demon=t(e.acc[1])[:3])
    with pytest.raises(TypeError, match="offset_selection_mask must be bool"):
        acc(offset_selection_mask=t(e.selection).float())
    with pytest.raises(ValueError, match=r"anchor_demon must be \[12, 1\]"):
        acc(anchor_demon=t(e.acc[1])[:3])
    with pytest.raises(ValueError, match=r"neural_opacity must be \[10, 1\]"):
        acc(neural_opacity=t(e.opacity)[:9])
    with pytest.raises(ValueError, match=r"viewspace_grad must be \[\d+, 3\]"):
        acc(viewspace_grad=t(e.grad)[:, :2])
    with pytest.raises(ValueError, match="opacity_accum is updated in place and must be contiguous"):
        acc(opacity_accum=torch.zeros(12, 2)[:, :1])
    with pytest.raises(ValueError, match="opacity_accum must be on the GPU"):
        acc()
    with pytest.raises(ValueError, match="on the GPU"):
        acc(radii=t(e.radii) > 0)
