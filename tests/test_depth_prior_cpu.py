"""The depth-prior loss without a GPU (include/bloomscene_depth_loss.h, bloomscene_amd/depth_loss.py): the header's
analytic gradient in float64 against float64 autograd of the restatement of tests/depth_prior_reference.py, the
batch-of-one CMD identity, the pinned spatial kernel, HuberL1's continuity across l1 = d, and every error the Python
layer raises before it touches a device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import depth_prior_reference as DR
import helpers as Hh
from bloomscene_amd import _capi
import bloomscene_amd.depth_loss as DL

SHAPES = ((2, 2), (3, 5), (5, 5), (12, 13))
WEIGHTS = {"all": (0.7, 0.3, 1.9), "value": (0.7, None, None), "domin": (None, 0.3, None), "smooth": (None, None, 1.9)}
# float64 carries 2^-53; the gradient divides by the depth range (O(1) here) and sums at most 156 pixels of 25 taps: the
# two evaluations of ONE formula differ by a few thousand roundings at the very most
F64_TOL = 1e-11


def _np(*ts):
    return [t.numpy() for t in ts]


@pytest.mark.parametrize("kind", ("smooth", "noise", "rendered"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_analytic_gradient_is_float64_autograd(shape, kind):
    D, P, rgb = DR.scene(kind, *shape)
    for which, (wv, wd, ws) in WEIGHTS.items():
        for norm in (True, False):
            ref = DR.autograd64(D, P, rgb, wv, wd, ws, norm, upstream=1.5)
            got = DR.evaluate(*_np(D, P, rgb), wv, wd, ws, norm, dt=np.float64, upstream=1.5)
            # the scene's promise: the maximum of |r - o| is unique, in float32 too
            assert got.cnt_M == 1 and DR.evaluate(*_np(D, P, rgb), wv, wd, ws, norm, dt=np.float32).cnt_M == 1
            assert np.abs(ref.grad).max() > 0
            err = Hh.max_err_over_scale(got.grad, ref.grad)
            assert err <= F64_TOL, (which, norm, err)
            for a, b in zip(got.out, ref.out):
                assert abs(a - b) <= F64_TOL * max(abs(b), 1.0), (which, norm, got.out, ref.out)


def test_border_pixels_of_the_smoothness_term_differ_from_the_interior_rule():
    """Within two pixels of the border A2 != -A1 (replicate padding maps several taps of one pixel onto one neighbour): the
    interior rule 2 * A1 must FAIL there against autograd, and the header's gather must pass (the test above)."""
    D, P, rgb = DR.scene("noise", 9, 10)
    ref = DR.autograd64(D, P, rgb, None, None, 1.0, False)
    r = D.double().numpy()
    pad = np.pad(r, 2, mode="edge")
    sk = DR.sk_table(np.float64)
    A1 = np.zeros_like(r)
    for i in range(5):
        for j in range(5):
            x = r - pad[i:i + 9, j:j + 10]
            A1 += sk[i, j] * np.exp(-np.abs(x) / 50) * (2 * x - np.sign(x) * x * x / 50)
    naive = 2 * A1 / r.size
    inner = np.zeros_like(r, dtype=bool)
    inner[2:-2, 2:-2] = True
    assert Hh.max_err_over_scale(naive[inner], ref.grad[inner]) <= F64_TOL
    assert np.abs(naive - ref.grad)[~inner].max() > 1e-3 * np.abs(ref.grad).max()


@pytest.mark.parametrize("shape", ((2, 2), (12, 13)), ids=lambda s: "x".join(map(str, s)))
def test_tied_extrema_get_equal_shares(shape):
    D, P, rgb = DR.scene("rendered", *shape)
    d = D.numpy()
    assert (d == d.min()).sum() >= 1 and (d == d.max()).sum() == 2 and d.min() == 0.0
    ref = DR.autograd64(D, P, rgb, 0.7, 0.3, 1.9, True)
    got = DR.evaluate(*_np(D, P, rgb), 0.7, 0.3, 1.9, True, dt=np.float64)
    assert got.cnt_max == 2 and got.cnt_min == (d == 0).sum()
    rg = (d.max().astype(np.float64) - d.min()) + 1e-8
    share = ref.grad - got.G / rg          # what autograd adds on top of the direct path
    for mask, want in ((d == d.min(), got.share_min), (d == d.max(), got.share_max)):
        assert np.abs(share[mask] - want).max() <= F64_TOL * np.abs(ref.grad).max()
        assert abs(want) > 0
    neither = (d != d.min()) & (d != d.max())
    assert np.abs(share[neither]).max() <= F64_TOL * np.abs(ref.grad).max()


def test_flat_scene_selects_no_zero_over_zero():
    D, P, rgb = DR.scene("flat", 5, 7)
    for dt in (np.float32, np.float64):
        got = DR.evaluate(*_np(D, P, rgb), 0.7, 0.3, 1.9, True, dt=dt)
        assert got.M == 0 and got.d == 0 and got.cnt_M == 35
        assert np.isfinite(got.h).all() and (got.h == 0).all() and np.isfinite(got.out).all()
        assert np.isfinite(got.grad).all() and (got.grad == 0).all()
    loss, (lv, ld, ls) = DR.restatement(D.double(), P.double(), rgb.double(), 0.7, 0.3, 1.9)
    assert lv.item() == 0.0 and ls.item() == 0.0 and abs(ld.item() - got.out[2]) <= 1e-12


@pytest.mark.parametrize("shape", ((1, 1), (3, 5), (40, 30)), ids=lambda s: "x".join(map(str, s)))
def test_batch_of_one_cmd_identity_and_k(shape):
    H, W = shape
    gen = torch.Generator().manual_seed(5)
    for scale in (1.0, 300.0, 3e6):       # the per-pixel clamp, the sum clamp and the input clamp each become active
        x1 = (torch.rand(1, H, W, generator=gen, dtype=torch.float64) - 0.5) * scale
        x2 = (torch.rand(1, H, W, generator=gen, dtype=torch.float64) - 0.5) * scale
        loop = DR.cmd(x1, x2).item()
        diff = torch.clamp(x1, -1e6, 1e6) - torch.clamp(x2, -1e6, 1e6)
        S = torch.clamp((diff.abs() + 1e-6) ** 2, max=1e6).sum().item()
        K = 4 * np.sqrt(H * W * 1e-6 ** 2 + 1e-6)
        assert abs(loop - (np.sqrt(min(S, 1e6) + 1e-6) + K)) <= 1e-12 * loop
    # the header's K (the fp32 1e-6) as evaluate() forms it
    got = DR.evaluate(x1[0].numpy(), x2[0].numpy(), np.zeros((H, W, 3)), None, 1.0, None, False, dt=np.float32)
    assert got.K == 4 * np.sqrt(H * W * float(np.float32(1e-6)) ** 2 + 1e-6)
    # any other batch: the central moments are no longer constants
    two = torch.rand(2, H, W, generator=gen, dtype=torch.float64)
    assert abs(DR.cmd(two, two.flip(0)).item() - DR.cmd(two[:1], two[1:]).item()) > 1e-9 or H * W == 1


def test_spatial_kernel_constants_are_torch_fp32():
    text = open(os.path.join(Hh.ROOT, "include", "bloomscene_depth_loss.h")).read()
    pinned = {int(k): v for k, v in re.findall(r"#define BSR_DEPTH_PRIOR_SK(\d) (0x[0-9a-fp.+-]+)f", text)}
    assert pinned == DR.SK_HEX
    sk = DR.spatial_kernel(torch.float32).numpy()
    assert sk.dtype == np.float32
    seen = set()
    for i in range(5):
        for j in range(5):
            k = (i - 2) ** 2 + (j - 2) ** 2
            seen.add(k)
            want = np.float32(float.fromhex(pinned[k]))
            assert float(want) == float.fromhex(pinned[k])                     # an fp32 literal
            assert sk[i, j].view(np.uint32) == want.view(np.uint32), (i, j, float(sk[i, j]).hex(), pinned[k])
    assert seen == set(pinned)
    assert (DR.sk_table(np.float32).view(np.uint32) == sk.view(np.uint32)).all()


def test_fp32_maps_of_the_header_are_the_torch_lines_bit_for_bit():
    for kind in DR.SCENES:
        D, P, rgb = DR.scene(kind, 12, 13)
        got = DR.evaluate(*_np(D, P, rgb), 1.0, 1.0, 1.0, True, dt=np.float32)
        r, o = DR.normalise(D), DR.normalise(P)
        l1 = (r - o).abs()
        d = 0.2 * l1.max()
        h = torch.where(l1 >= d, l1, ((r - o) ** 2 + d ** 2) / (2 * d))
        for name, a, b in (("r", got.r, r), ("o", got.o, o), ("h", got.h, h)):
            assert (a.view(np.uint32) == b.numpy().view(np.uint32)).all(), (kind, name)


def test_huber_is_continuous_across_the_threshold():
    """value and gradient at l1 = d (1 -/+ eps): the two branches meet ((d^2 + d^2) / 2d = d, e / d = sign(e)) and the
    part through d vanishes there (1/2 - e^2 / 2d^2 = 0)."""
    rng = np.random.RandomState(3)
    P = np.zeros((4, 5))
    rgb = rng.rand(4, 5, 3)
    base = 0.05 + 0.1 * rng.rand(4, 5)           # quadratic branch
    base[1, 2] = 1.0                              # M = 1, d = 0.2
    base[3, 3] = 0.5                              # linear branch
    sides = []
    for eps in (-1e-9, 1e-9):
        D = base.copy()
        D[2, 1] = 0.2 * (1 + eps)
        got = DR.evaluate(D, P, rgb, 1.0, None, None, False, dt=np.float64)
        assert bool(got.l1[2, 1] >= got.d) == (eps > 0)
        ref = DR.autograd64(*(torch.from_numpy(a) for a in (D, P, rgb)), 1.0, None, None, False)
        assert Hh.max_err_over_scale(got.grad, ref.grad) <= F64_TOL
        sides.append(got)
    lo, hi = sides
    assert abs(lo.h[2, 1] - hi.h[2, 1]) <= 1e-9 and abs(lo.out[1] - hi.out[1]) <= 1e-9
    assert np.abs(lo.grad - hi.grad).max() <= 1e-8 * np.abs(hi.grad).max()


# ---------------------------------------------------------------- the Python layer, before any device
def _inputs(H=6, W=7):
    return torch.rand(H, W), torch.rand(H, W), torch.rand(H, W, 3)


def test_errors_in_order_before_the_device_is_touched():
    D, P, rgb = _inputs()
    f = DL.depth_prior_loss
    # dtype first -- even with a shape that is wrong and a gradient that is refused
    with pytest.raises(TypeError, match="float32"):
        f(D.double(), P[:2].requires_grad_(True), rgb, value=1.0)
    with pytest.raises(TypeError, match="float32"):
        f(D, P, rgb.half(), value=1.0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        f(D.numpy(), P, rgb, value=1.0)
    with pytest.raises(TypeError, match="float32"):
        DL.depth_prior_maps(D, P.double(), rgb)
    # then what is not implemented -- even with a wrong shape
    with pytest.raises(NotImplementedError, match="prior_depth"):
        f(D, P[:2].clone().requires_grad_(True), rgb, value=1.0)
    with pytest.raises(NotImplementedError, match="rgb"):
        f(D, P, rgb.clone().requires_grad_(True), value=1.0)
    with pytest.raises(NotImplementedError, match="batch of one"):
        f(torch.rand(2, 6, 7), torch.rand(2, 6, 7), rgb, domin=1.0)
    # then shapes
    with pytest.raises(ValueError, match="prior_depth"):
        f(D, P[:2], rgb, value=1.0)
    with pytest.raises(ValueError, match="rgb"):
        f(D, P, rgb[:, :, :2], value=1.0)
    with pytest.raises(ValueError, match="render_depth"):
        f(D[0], P[0], rgb, smooth=1.0)
    with pytest.raises(ValueError, match="at least 2"):
        f(torch.rand(1, 7), torch.rand(1, 7), torch.rand(1, 7, 3), value=1.0)
    with pytest.raises(ValueError, match="at least 2"):
        f(torch.rand(7, 1), torch.rand(7, 1), torch.rand(7, 1, 3), value=1.0, smooth=1.0)
    big = torch.zeros(1, 1).expand(1 << 16, 1 << 15)              # 2^31 pixels, one element of memory
    with pytest.raises(ValueError, match="2\\^31"):
        f(big, big, torch.zeros(1, 1, 1).expand(1 << 16, 1 << 15, 3), smooth=1.0)
    # the device last: everything else is right, and there is no CPU path
    for kw in ({"value": 1.0}, {"domin": 1.0}, {"smooth": 1.0}, {"value": 1.0, "domin": 2.0, "smooth": 3.0}):
        with pytest.raises(ValueError, match="GPU"):
            f(D, P, rgb, **kw)
        with pytest.raises(ValueError, match="GPU"):
            f(D[None], P[None], rgb[None], **kw)
    with pytest.raises(ValueError, match="GPU"):
        f(torch.rand(1, 7), torch.rand(1, 7), None, smooth=1.0)     # H = 1 is fine without the value term
    with pytest.raises(ValueError, match="GPU"):
        DL.depth_prior_maps(D, P, rgb)
    with pytest.raises(TypeError, match="weight"):
        f(D, P, rgb, value=torch.tensor(1.0))


def test_drop_ins_keep_the_reference_signatures_and_name_what_they_refuse():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name not in ("self", "kwargs")]

    E = inspect.Parameter.empty
    assert params(DL.HuberL1.__init__) == [("tresh", 0.2), ("implementation", "scalar")]
    assert params(DL.HuberL1.forward) == [("pred", E), ("gt", E), ("rgb", E)]
    assert params(DL.CMD.forward) == [("x1", E), ("x2", E), ("n_moments", 5)]
    assert params(DL.bilateral_filter) == [("depth", E), ("spatial_sigma", 2.0), ("color_sigma", 5.0), ("kernel_size", 5)]
    assert params(DL.depth_prior_loss) == [("render_depth", E), ("prior_depth", E), ("rgb", E), ("value", None), ("domin", None),
                                           ("smooth", None), ("normalise", True), ("return_terms", False)]
    D, P, rgb = _inputs()
    with pytest.raises(NotImplementedError, match="tresh"):
        DL.HuberL1(tresh=0.3)
    with pytest.raises(NotImplementedError, match="implementation"):
        DL.HuberL1(implementation="per-pixel")
    with pytest.raises(NotImplementedError, match="n_moments"):
        DL.CMD()(D[None], P[None], n_moments=3)
    with pytest.raises(NotImplementedError, match="batch of one"):
        DL.CMD()(torch.rand(2, 6, 7), torch.rand(2, 6, 7))
    for kw, name in (({"spatial_sigma": 1.0}, "spatial_sigma"), ({"color_sigma": 0.1}, "color_sigma"), ({"kernel_size": 3}, "kernel_size")):
        with pytest.raises(NotImplementedError, match=name):
            DL.bilateral_filter(D[None], **kw)
    with pytest.raises(NotImplementedError, match="batch of one"):
        DL.bilateral_filter(torch.rand(2, 6, 7))
    # dtype before NotImplementedError; the device last
    with pytest.raises(TypeError):
        DL.bilateral_filter(D[None].double(), color_sigma=0.1)
    with pytest.raises(TypeError):
        DL.CMD()(D[None].double(), P[None], n_moments=3)
    with pytest.raises(TypeError):
        DL.HuberL1()(D, P.double(), rgb)
    with pytest.raises(NotImplementedError, match="gradient to"):
        DL.HuberL1()(D.reshape(1, 6, 7, 1), P.reshape(1, 6, 7, 1).requires_grad_(True), rgb[None])
    with pytest.raises(ValueError, match="GPU"):
        DL.HuberL1()(D.reshape(6, 7, 1), P.reshape(1, 6, 7, 1), rgb[None])       # the reference's own shapes
    with pytest.raises(ValueError, match="GPU"):
        DL.CMD()(D[None], P[None, None])
    with pytest.raises(ValueError, match="GPU"):
        DL.bilateral_filter(D[None], spatial_sigma=2.0, color_sigma=5.0)


def test_scratch_sizing_and_entry_points():
    lib = _capi.lib()
    for name in ("bsr_depth_prior_scratch_bytes", "bsr_depth_prior_forward", "bsr_depth_prior_backward"):
        assert name in _capi.SIGNATURES and hasattr(lib, name)
    assert lib.bsr_version() == 4
    tiles = lambda H, W: ((H + 15) // 16) * ((W + 31) // 32)
    for H, W in ((1, 1), (2, 2), (512, 512), (1080, 1920)):
        n = lib.bsr_depth_prior_scratch_bytes(H, W)
        assert n % 256 == 0 and n == 256 + 1024 * 32 + -(-min(tiles(H, W), 16384) * 40 // 256) * 256
    assert lib.bsr_depth_prior_scratch_bytes(0, 5) == 0 and lib.bsr_depth_prior_scratch_bytes(5, -1) == 0
    assert lib.bsr_depth_prior_scratch_bytes(1 << 16, 1 << 15) == 0


# ---------------------------------------------------------------- the scenes built for one branch each (DR.EDGE_SCENES)
TIED = (("tied_M", (17, 33), 3, 2), ("tied_M", (37, 53), 3, 2), ("tied_wide", (80, 80), 5, 4))


@pytest.mark.parametrize("kind,shape,n_neg,n_pos", TIED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tied_scenes_have_the_ties_they_were_built_for(kind, shape, n_neg, n_pos):
    """What the GPU tests of the tied maximum rely on, so that none passes vacuously: cnt_M, cnt_min, cnt_max in fp32 and
    float64 alike, both signs of e at the tied pixels, the runner-up at half of M at most, one gradient per sign class in
    the fp32 evaluation of the header, the header's equal shares equal to float64 autograd (torch.max splits the gradient
    of a tied maximum evenly) -- and for tied_wide every tie spread over the four workgroups of the linear reductions."""
    D, P, rgb = DR.scene(kind, *shape)
    neg, pos = DR.tied_pixels(kind, *shape)
    assert (len(neg), len(pos)) == (n_neg, n_pos)
    d, p = D.numpy().reshape(-1), P.numpy().reshape(-1)
    assert d.min() == 0 and d.max() == 4 and p.min() == 0 and p.max() == 4
    assert sorted(np.flatnonzero(d == 0)) == sorted(neg) == sorted(np.flatnonzero(p == 4))
    assert sorted(np.flatnonzero(d == 4)) == sorted(pos) == sorted(np.flatnonzero(p == 0))
    if kind == "tied_wide":
        assert shape[0] * shape[1] > 3 * 2048                      # four workgroups (BSR_DEPTH_LIN_PER_BLOCK pixels each)
        for group in (neg, pos):
            assert {(i // 256) % 4 for i in group} == {0, 1, 2, 3}
    else:
        assert shape[0] * shape[1] <= 2048
    for norm in (True, False):
        for cfg in ("all", "value"):
            w = WEIGHTS[cfg]
            ref = DR.autograd64(D, P, rgb, *w, norm)
            for dt in (np.float64, np.float32):
                ev = DR.evaluate(*_np(D, P, rgb), *w, norm, dt=dt)
                assert ev.cnt_M == n_neg + n_pos >= 5
                if norm:
                    assert (ev.cnt_min, ev.cnt_max) == (n_neg, n_pos)
                e = (ev.r - ev.o).reshape(-1)
                assert (e[neg] == -ev.M).all() and (e[pos] == ev.M).all() and ev.M > 0
                others = np.ones(e.size, bool)
                others[neg + pos] = False
                assert np.abs(e[others]).max() <= 0.5 * ev.M
                g = ev.grad.reshape(-1)
                for group in (neg, pos):
                    assert (g[group] == g[group[0]]).all() and g[group[0]] != 0
                if dt == np.float64:
                    assert Hh.max_err_over_scale(ev.grad, ref.grad) <= F64_TOL, (norm, cfg)


def test_clamp_gate_scenes_open_and_close_the_gates_they_were_built_for():
    """The distribution term alone, no normalisation.  5 x 5: S < 1e6 (the sum gate is open), the three pixels beyond
    +-1e6 are closed by |r| <= 1e6, the two exactly at the bound are open -- torch.clamp passes the gradient at the bound
    -- like everything else.  1 x 1 with D = 2000, P = 0: S is exactly 1e6, open, and the pixel's own t t <= 1e6 is
    closed; no other input separates the two gates."""
    D, P = DR.clamp_gate_scene()
    rgb = torch.zeros(5, 5, 3)
    beyond = np.zeros((5, 5), bool)
    beyond[0, 0] = beyond[1, 2] = beyond[4, 4] = True
    assert (np.abs(D.numpy()) > 1e6).sum() == 3 and (np.abs(D.numpy())[beyond] > 1e6).all()
    assert D[2, 2].item() == 1e6 and D[3, 1].item() == -1e6
    ref = DR.autograd64(D, P, rgb, None, 1.0, None, False)
    for dt in (np.float64, np.float32):
        ev = DR.evaluate(*_np(D, P, rgb), None, 1.0, None, False, dt=dt)
        assert ev.S < 1e6 and (ev.gate == ~beyond).all()
        assert not ev.grad[beyond].any() and ev.grad[~beyond].all()
    assert not ref.grad[beyond].any() and ref.grad[2, 2] != 0 and ref.grad[3, 1] != 0
    assert Hh.max_err_over_scale(DR.evaluate(*_np(D, P, rgb), None, 1.0, None, False, dt=np.float64).grad, ref.grad) <= F64_TOL
    one = DR.evaluate(np.full((1, 1), 2000.0), np.zeros((1, 1)), np.zeros((1, 1, 3)), None, 1.0, None, False, dt=np.float32)
    assert one.S == 1e6 and not one.gate.any() and not one.grad.any()
    ref = DR.autograd64(torch.full((1, 1), 2000.0), torch.zeros(1, 1), torch.zeros(1, 1, 3), None, 1.0, None, False)
    assert not ref.grad.any() and abs(ref.out[2] - (np.sqrt(1e6 + 1e-6) + 4 * np.sqrt(1e-12 + 1e-6))) <= 1e-9


@pytest.mark.parametrize("shape", ((1, 1), (1, 40), (40, 1), (2, 40)), ids=lambda s: "x".join(map(str, s)))
def test_thin_shapes_without_the_value_term(shape):
    """H = 1 or W = 1 is legal with the value term off: the header's gather of A2 then has both border rules on at once."""
    for kind in ("noise", "rendered"):
        D, P, rgb = DR.scene(kind, *shape)
        ref = DR.autograd64(D, P, rgb, None, 0.3, 1.9, True)
        got = DR.evaluate(*_np(D, P, rgb), None, 0.3, 1.9, True, dt=np.float64)
        assert Hh.max_err_over_scale(got.grad, ref.grad) <= F64_TOL or not ref.grad.any()
        assert np.abs(got.grad - ref.grad).max() <= F64_TOL * max(np.abs(ref.grad).max(), 1.0)
        for a, b in zip(got.out, ref.out):
            assert abs(a - b) <= F64_TOL * max(abs(b), 1.0)


def test_native_entry_points_refuse_the_value_term_on_a_thin_shape_with_the_headers_words():
    import threading
    lib = _capi.lib()
    seen = []

    def calls():             # (the error string belongs to the calling thread: this one's dies with it)
        for H, W in ((1, 40), (40, 1), (1, 1)):
            for fn in (lib.bsr_depth_prior_forward, lib.bsr_depth_prior_backward):
                rc = fn(H, W, None, None, None, 0, 0, 0, 1 | 4, 1.0, 1.0, 1.0, 1, None, None, None, None, None)
                seen.append((rc, f"the value term needs H, W >= 2 (got {H}, {W})" in _capi.last_error()))

    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert seen == [(1, True)] * 6, seen


def test_near_flat_scene_spans_three_units_of_the_depth():
    for shape in ((17, 33), (37, 53)):
        D, P, rgb = DR.scene("near_flat", *shape)
        d = D.numpy()
        assert d.max() - d.min() == 3 * np.spacing(np.float32(2.0)) and len(np.unique(d)) == 4
        ev = DR.evaluate(*_np(D, P, rgb), 0.7, 0.3, 1.9, True, dt=np.float32)
        assert ev.cnt_M == 1 and ev.cnt_min > 50 and ev.cnt_max > 50
        assert abs(float(d.max() - d.min()) / 1e-8 - 71.5) < 1          # (the 1e-8 of the range is 1.4 % of it)
