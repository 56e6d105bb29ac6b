"""The depth-prior loss on the GPU (include/bloomscene_depth_loss.h, bloomscene_amd/depth_loss.py) against
tests/depth_prior_reference.py: the maps r, o, h bit for bit with the numpy evaluation of the header, everything that
holds a transcendental or a sum against float64 autograd of the restatement, with the fp32 eager restatement on the same
GPU as the measure of what fp32 can do:

    kernel error <= 2 x eager error + 2^-23        (helpers.max_err_over_scale, pooled over the small shapes per scene)
    |scalar - float64| <= 2 x |eager - float64| + one fp32 unit of the value

(two legal fp32 roundings of one formula differ by chance, a wrong term by orders of magnitude; the floor keeps an
accidentally exact eager run at a tiny shape from failing a correct kernel).

Shapes, relative to the kernels' tile of 32 x 16 pixels: (2, 2) every bilateral tap but the centre is padding; (3, 5);
(5, 5); exactly one tile; one pixel over a tile each way; (37, 53) ragged, multi-tile, halos crossing tile edges both
ways; narrow and tall; and (512, 512) once, 512 workgroups for the tickets.  Every (shape, scene) is evaluated once and
shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_prior_reference as DR
import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TW, TH = 32, 16      # BSR_DEPTH_TW, BSR_DEPTH_TH of csrc/depth_loss.hip
SMALL = ((2, 2), (3, 5), (5, 5), (TH, TW), (TH + 1, TW + 1), (37, 53), (2 * TH + 3, 2))
BIG = (512, 512)
KINDS = ("smooth", "noise", "rendered")          # (flat has its own test: float64 autograd is 0 / 0 there)
W3 = (0.7, 0.3, 1.9)
CONFIGS = {"all": W3, "value": (0.7, None, None), "domin": (None, 0.3, None), "smooth": (None, None, 1.9),
           "ds": (None, 0.3, 1.9)}
FLOOR = 2.0 ** -23


def _L():
    import bloomscene_amd.depth_loss as L
    return L


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _unit(x):
    return float(np.spacing(np.float32(abs(x))))


def _run(D, P, rgb, w=W3, norm=True, upstream=1.0):
    """depth_prior_loss forward + backward on a fresh leaf -> (out[4] numpy float32, grad numpy)"""
    leaf = D.clone().requires_grad_(True)
    loss, terms = _L().depth_prior_loss(leaf, P, rgb, *w, normalise=norm, return_terms=True)
    (loss if upstream == 1.0 else upstream * loss).backward()
    return np.array([loss.item()] + [t.item() for t in terms], dtype=np.float32), leaf.grad.cpu().numpy()


def _eager(D, P, rgb, w=W3, norm=True, upstream=1.0):
    """the fp32 restatement on the GPU, forward + autograd -> (out[4] as floats, grad numpy)"""
    leaf = D.clone().requires_grad_(True)
    loss, terms = DR.restatement(leaf, P, rgb, *w, norm)
    (upstream * loss).backward()
    return [loss.item()] + [t.item() for t in terms], leaf.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _scene(shape, kind):
    D, P, rgb = DR.scene(kind, *shape, seed=1)
    return SimpleNamespace(D=D, P=P, rgb=rgb, Dd=D.to(DEV), Pd=P.to(DEV), rgbd=rgb.to(DEV))


@functools.lru_cache(maxsize=None)
def _case(shape, kind, cfg="all", norm=True, upstream=1.0):
    """float64 autograd, the eager fp32 lines and the kernels for one call, computed once and left unchanged"""
    s = _scene(shape, kind)
    w = CONFIGS[cfg]
    c = SimpleNamespace(shape=shape, kind=kind, s=s)
    c.ref = DR.autograd64(s.D, s.P, s.rgb, *w, norm, upstream=upstream)
    c.eager_out, c.eager_grad = _eager(s.Dd, s.Pd, s.rgbd, w, norm, upstream)
    c.out, c.grad = _run(s.Dd, s.Pd, s.rgbd, w, norm, upstream)
    c.err = Hh.max_err_over_scale(c.grad, c.ref.grad)
    c.eager_err = Hh.max_err_over_scale(c.eager_grad, c.ref.grad)
    return c


def _check_scalars(label, out, eager_out, ref_out):
    for name, got, eager, exact in zip(("loss", "Lv", "Ld", "Ls"), out, eager_out, ref_out):
        bound = 2 * abs(eager - exact) + _unit(exact)
        print(f"{label} {name}: kernel {float(got)!r} eager {eager!r} float64 {exact!r} |kernel - f64| {abs(float(got) - exact):.3e} "
              f"bound {bound:.3e}")
        assert abs(float(got) - exact) <= bound, (label, name, float(got), eager, exact)


def _items(result):
    loss, terms = result
    return [loss.item()] + [t.item() for t in terms]


def _ids(shape):
    return "x".join(map(str, shape))


@pytest.mark.parametrize("shape,kind", [(s, k) for s in SMALL for k in DR.SCENES] + [(BIG, "noise")],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_maps(shape, kind):
    s = _scene(shape, kind)
    r, o, h, b = (t.cpu().numpy() for t in _L().depth_prior_maps(s.Dd, s.Pd, s.rgbd))
    ev = DR.evaluate(s.D.numpy(), s.P.numpy(), s.rgb.numpy(), *W3, dt=np.float32)
    for name, got, want in (("r", r, ev.r), ("o", o, ev.o), ("h", h, ev.h)):
        assert got.shape == shape and np.isfinite(want).all()
        assert (_bits(got) == _bits(want)).all(), (name, float(np.abs(got - want).max()))
    # the bilateral map holds an exp: against float64, with the eager fp32 map as the measure
    exact = DR.bilateral_map(DR.normalise(s.D.double())).numpy()
    eager = DR.bilateral_map(DR.normalise(s.Dd)).cpu().numpy()
    err, eager_err = Hh.max_err_over_scale(b, exact), Hh.max_err_over_scale(eager, exact)
    print(f"bilateral map {shape} {kind}: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR
    if kind == "flat":
        assert not b.any() and not h.any() and not r.any()


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_against_float64_autograd_pooled_over_the_small_shapes(kind):
    cases = [_case(shape, kind) for shape in SMALL]
    for c in cases:
        assert c.grad.shape == c.shape and np.isfinite(c.grad).all() and np.abs(c.ref.grad).max() > 0
        print(f"gradient {c.shape} {kind}: kernel {c.err:.3e} eager {c.eager_err:.3e}")
    err, eager_err = max(c.err for c in cases), max(c.eager_err for c in cases)
    print(f"gradient pooled {kind}: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR


def test_gradient_and_scalars_at_512_for_the_tickets():
    c = _case(BIG, "noise")
    print(f"gradient {BIG}: kernel {c.err:.3e} eager {c.eager_err:.3e}")
    assert c.err <= 2 * c.eager_err + FLOOR
    _check_scalars("512x512 noise", c.out, c.eager_out, c.ref.out)


@pytest.mark.parametrize("kind", DR.SCENES)
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_scalars(shape, kind):
    if kind == "flat":
        s = _scene(shape, kind)
        out, grad = _run(s.Dd, s.Pd, s.rgbd)
        eager_out = _items(DR.restatement(s.Dd, s.Pd, s.rgbd, *W3))
        exact = _items(DR.restatement(s.D.double(), s.P.double(), s.rgb.double(), *W3))
        _check_scalars(f"{shape} flat", out, eager_out, exact)
        assert out[1] == 0 and out[3] == 0
        # M = 0: the 0 / 0 branch is never selected, and every sign is sign(0) = 0
        assert np.isfinite(grad).all() and not grad.any()
        return
    c = _case(shape, kind)
    _check_scalars(f"{shape} {kind}", c.out, c.eager_out, c.ref.out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", ("value", "domin", "smooth"))
def test_each_term_alone(cfg, kind):
    cases = [_case(shape, kind, cfg) for shape in ((5, 5), (TH + 1, TW + 1), (37, 53))]
    for c in cases:
        _check_scalars(f"{c.shape} {kind} {cfg}", c.out, c.eager_out, c.ref.out)
        off = [k for k, w in zip((1, 2, 3), CONFIGS[cfg]) if w is None]
        assert all(c.out[k] == 0 for k in off)
    err, eager_err = max(c.err for c in cases), max(c.eager_err for c in cases)
    print(f"gradient pooled {kind} {cfg}: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR


@pytest.mark.parametrize("kind", KINDS)
def test_non_unit_upstream(kind):
    cases = [_case(shape, kind, "all", True, 3.5) for shape in ((5, 5), (TH + 1, TW + 1), (37, 53))]
    for c in cases:
        _check_scalars(f"{c.shape} {kind} upstream", c.out, c.eager_out, c.ref.out)
        assert (_bits(c.out) == _bits(_case(c.shape, kind).out)).all()
    err, eager_err = max(c.err for c in cases), max(c.eager_err for c in cases)
    print(f"gradient pooled {kind} upstream 3.5: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR


@pytest.mark.parametrize("kind", KINDS)
def test_drop_ins_without_normalisation(kind):
    L = _L()
    calls = {"value": lambda D, P, rgb: L.HuberL1(tresh=0.2)(D.reshape(1, *D.shape, 1), P.reshape(1, *P.shape, 1), rgb[None]),
             "domin": lambda D, P, rgb: L.CMD()(D[None], P[None, None], n_moments=5),
             "smooth": lambda D, P, rgb: L.bilateral_filter(D[None], spatial_sigma=2.0, color_sigma=5.0)}
    for cfg, call in calls.items():
        w = tuple(None if v is None else 1.0 for v in CONFIGS[cfg])
        pooled = []
        for shape in ((5, 5), (TH + 1, TW + 1), (37, 53)):
            s = _scene(shape, kind)
            ref = DR.autograd64(s.D, s.P, s.rgb, *w, False)
            eager_out, eager_grad = _eager(s.Dd, s.Pd, s.rgbd, w, False)
            leaf = s.Dd.clone().requires_grad_(True)
            val = call(leaf, s.Pd, s.rgbd)
            assert val.dim() == 0 and val.requires_grad
            val.backward()
            k = 1 + ("value", "domin", "smooth").index(cfg)
            bound = 2 * abs(eager_out[k] - ref.out[k]) + _unit(ref.out[k])
            print(f"{cfg} drop-in {shape} {kind}: kernel {val.item()!r} eager {eager_out[k]!r} float64 {ref.out[k]!r}")
            assert abs(val.item() - ref.out[k]) <= bound
            pooled.append((Hh.max_err_over_scale(leaf.grad.cpu().numpy(), ref.grad), Hh.max_err_over_scale(eager_grad, ref.grad)))
        err, eager_err = max(p[0] for p in pooled), max(p[1] for p in pooled)
        print(f"gradient pooled {kind} {cfg} drop-in: kernel {err:.3e} eager {eager_err:.3e}")
        assert err <= 2 * eager_err + FLOOR


@pytest.mark.parametrize("shape", ((TH + 1, TW + 1), (37, 53)), ids=_ids)
def test_tied_minima_get_identical_shares(shape):
    s = _scene(shape, "rendered")
    d = s.D.numpy()
    tied = d == 0.0
    assert tied.sum() == (shape[0] // 3) * (shape[1] // 3) and (d == d.max()).sum() == 2
    # the smoothness term alone: a tied pixel with nothing but zeros in its window has G = 0, so its gradient IS the share
    w = CONFIGS["smooth"]
    out, grad = _run(s.Dd, s.Pd, s.rgbd, w)
    ev = DR.evaluate(d, s.P.numpy(), s.rgb.numpy(), *w, dt=np.float64)
    deep = np.zeros_like(tied)
    deep[:shape[0] // 3 - 2, :shape[1] // 3 - 2] = True
    assert deep.sum() > 4 and not ev.G[deep].any()
    shares = _bits(grad[deep])
    assert (shares == shares[0]).all() and grad[deep][0] != 0
    alone = _case(shape, "rendered", "smooth")
    assert (_bits(alone.grad) == _bits(grad)).all()
    exact, eager = alone.ref.grad[deep][0], float(alone.eager_grad[deep][0])
    assert abs(exact - ev.share_min) <= 1e-11 * abs(exact)
    print(f"share of a tied minimum {shape}: kernel {float(grad[deep][0])!r} eager {eager!r} float64 {exact!r}")
    assert abs(float(grad[deep][0]) - exact) <= 2 * abs(eager - exact) + FLOOR * abs(exact)
    # all three terms: the totals over the tied minima and over the tied maxima against float64
    c = _case(shape, "rendered")
    for mask in (tied, d == d.max()):
        exact, got, eager = c.ref.grad[mask].sum(), c.grad[mask].astype(np.float64).sum(), c.eager_grad[mask].astype(np.float64).sum()
        bound = 2 * abs(eager - exact) + FLOOR * np.abs(c.ref.grad[mask]).sum()
        print(f"tied total {shape}: kernel {got!r} eager {eager!r} float64 {exact!r}")
        assert abs(got - exact) <= bound


def test_clamp_gate_at_1080p():
    """Only the distribution term, D and P at opposite extremes: S > 1e6, so the term is sqrt(1e6 + 1e-6) + K and torch's
    clamp rule passes no gradient at all."""
    H, W = 1080, 1920
    rng = np.random.RandomState(11)
    D = (0.01 * rng.rand(H, W)).astype(np.float32)
    P = (1.0 - 0.01 * rng.rand(H, W)).astype(np.float32)
    D[5, 7], P[9, 3] = 1.0, 0.0
    Dt, Pt = torch.from_numpy(D), torch.from_numpy(P)
    # the restatement itself crosses 1e6 (CPU, fp32 and float64)
    for t in (torch.float32, torch.float64):
        r, o = DR.normalise(Dt.to(t)), DR.normalise(Pt.to(t))
        assert torch.clamp(((r - o).abs() + 1e-6) ** 2, max=1e6).sum().item() > 1e6
    leaf = Dt.to(DEV).requires_grad_(True)
    loss, (lv, ld, ls) = _L().depth_prior_loss(leaf, Pt.to(DEV), None, domin=1.0, return_terms=True)
    loss.backward()
    K = 4 * np.sqrt(H * W * float(np.float32(1e-6)) ** 2 + 1e-6)
    want = np.sqrt(1e6 + 1e-6) + K
    assert abs(ld.item() - want) <= _unit(want) and _bits(loss.item()) == _bits(ld.item())
    assert lv.item() == 0 and ls.item() == 0
    assert not leaf.grad.any().item()


def test_combined_and_single_term_runs_agree_bit_for_bit_and_runs_repeat():
    for kind in KINDS:
        c = _case((37, 53), kind)
        for k, cfg in ((1, "value"), (2, "domin"), (3, "smooth")):
            assert _bits(c.out[k]) == _bits(_case((37, 53), kind, cfg).out[k]), (kind, cfg)
        out, grad = _run(c.s.Dd, c.s.Pd, c.s.rgbd)
        assert (_bits(out) == _bits(c.out)).all() and (_bits(grad) == _bits(c.grad)).all()
    c = _case(BIG, "noise")
    out, grad = _run(c.s.Dd, c.s.Pd, c.s.rgbd)
    assert (_bits(out) == _bits(c.out)).all() and (_bits(grad) == _bits(c.grad)).all()


def test_transposed_rgb_view_is_read_in_place():
    """The reference hands HuberL1 gt_image.permute(2, 1, 0): a [C, W, H] image seen as [H, W, 3] with strides (1, H, W H)."""
    for shape in ((37, 37), (37, 53)):
        c = _case((37, 53), "noise") if shape == (37, 53) else None
        s = _scene(shape, "noise")
        chw = s.rgbd.permute(2, 1, 0).contiguous()
        view = chw.permute(2, 1, 0)
        assert view.shape == s.rgbd.shape and not view.is_contiguous() and view.stride() == (1, shape[0], shape[0] * shape[1])
        assert torch.equal(view, s.rgbd)
        out_v, grad_v = _run(s.Dd, s.Pd, view)
        out_c, grad_c = _run(s.Dd, s.Pd, view.contiguous())
        assert (_bits(out_v) == _bits(out_c)).all() and (_bits(grad_v) == _bits(grad_c)).all()
        if c is not None:
            assert (_bits(out_v) == _bits(c.out)).all() and (_bits(grad_v) == _bits(c.grad)).all()
        # [1, H, W] depths and a [1, H, W, 3] image are the same call
        out_b, grad_b = _run(s.Dd[None], s.Pd[None], view[None])
        assert (_bits(out_b) == _bits(out_v)).all() and (_bits(grad_b[0]) == _bits(grad_v)).all()


def test_through_autograd():
    L = _L()
    c = _case((37, 53), "smooth")
    s = c.s
    x = (s.Dd * 2).requires_grad_(True)          # the depth comes out of an upstream op (x / 2 and g / 2 are exact)
    loss, terms = L.depth_prior_loss(x * 0.5, s.Pd, s.rgbd, *W3, return_terms=True)
    assert loss.dim() == 0 and loss.requires_grad and _bits(loss.item()) == _bits(c.out[0])
    assert type(loss.grad_fn).__name__ == "_DepthPriorBackward" and not any(t.requires_grad for t in terms)
    loss.backward()
    assert (_bits(x.grad.cpu().numpy()) == _bits(np.float32(0.5) * c.grad)).all()
    with pytest.raises(NotImplementedError):
        L.depth_prior_loss(s.Dd, s.Pd.clone().requires_grad_(True), s.rgbd, value=1.0)
    with pytest.raises(NotImplementedError):
        L.depth_prior_loss(s.Dd, s.Pd, s.rgbd.clone().requires_grad_(True), value=1.0)
    plain = L.depth_prior_loss(s.Dd, s.Pd, s.rgbd, *W3)
    assert not plain.requires_grad and _bits(plain.item()) == _bits(c.out[0])


def test_forward_and_backward_replay_from_a_graph_without_a_host_wait():
    """Forward and backward captured with torch.cuda.graph after one warm-up call (capture raises on any host wait) and
    replayed on new depth values: bit-equal to the direct call."""
    L = _L()
    shape = (37, 53)
    c, c2 = _case(shape, "smooth"), _case(shape, "rendered", "all", True, 3.5)
    D = c.s.Dd.clone().requires_grad_(True)
    P = c.s.Pd.clone()
    rgb = c.s.rgbd.clone()

    def step():
        loss, (lv, ld, ls) = L.depth_prior_loss(D, P, rgb, *W3, return_terms=True)
        grad, = torch.autograd.grad(3.5 * loss, [D])
        return loss, lv, ld, ls, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                           # the warm-up: loads the library
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():                                # new values in the captured tensors
        D.copy_(c2.s.Dd)
        P.copy_(c2.s.Pd)
        rgb.copy_(c2.s.rgbd)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.detach().clone() for t in captured]
    direct = step()
    torch.cuda.synchronize()
    for a, b in zip(replayed, direct):
        assert torch.equal(a, b.detach())
    assert (_bits(replayed[4].cpu().numpy()) == _bits(c2.grad)).all()
    assert (_bits(np.array([t.item() for t in replayed[:4]])) == _bits(c2.out)).all()


def test_library_owns_no_device_memory_and_no_grad_keeps_nothing():
    """Every device byte of a forward + backward comes from the caller, here torch's allocator; under no_grad nothing of
    the size of the image is allocated (the backward's only large buffer is the gradient)."""
    L = _L()
    _case((2, 2), "noise")                               # library and streams: set up
    H, W = 1080, 1920
    gen = torch.Generator(device=DEV).manual_seed(3)
    D = torch.rand((H, W), device=DEV, generator=gen).requires_grad_(True)
    P = torch.rand((H, W), device=DEV, generator=gen)
    rgb = torch.rand((3, W, H), device=DEV, generator=gen).permute(2, 1, 0)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    for wanted in (False, True):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if wanted:
            loss = L.depth_prior_loss(D, P, rgb, *W3)
            loss.backward()
        else:
            with torch.no_grad():
                loss = L.depth_prior_loss(D, P, rgb, *W3)
            assert not loss.requires_grad
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        assert (peak >= H * W * 4) == wanted, (wanted, peak)
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    # (growth only: the HIP runtime may release memory of its own meanwhile)
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    assert torch.isfinite(loss).item() and torch.isfinite(D.grad).all().item() and D.grad.any().item()
    lib = __import__("bloomscene_amd._capi", fromlist=["lib"]).lib()
    assert lib.bsr_depth_prior_scratch_bytes(H, W) == 256 + 1024 * 32 + -(-68 * 60 * 40 // 256) * 256


def test_end_to_end_through_the_rasterizer():
    """GaussianRasterizer(depth_gradient=True) -> depth_prior_loss -> backward(): finite, non-zero gradients at the
    Gaussians' means, equal to feeding the rasterizer's backward the loss's own depth gradient by hand."""
    from bloomscene_amd import GaussianRasterizer
    L = _L()
    c = Hh.make_case(P=300, W=64, H=48, deg=1, seed=4, scale_mul=6.0)
    gen = torch.Generator().manual_seed(8)
    prior = (1.0 + 3.0 * torch.rand(48, 64, generator=gen)).to(DEV)
    gt = torch.rand(3, 48, 64, generator=gen).to(DEV)

    def render():
        leaves = [t.to(DEV).clone().requires_grad_(True) for t in (c.means3D, c.opacities, c.shs, c.scales, c.rotations)]
        means2D = torch.zeros_like(leaves[0], requires_grad=True)
        rast = GaussianRasterizer(raster_settings=Hh.hip_settings(c, torch.device(DEV)), depth_gradient=True)
        color, radii, depth = rast(means3D=leaves[0], means2D=means2D, opacities=leaves[1], shs=leaves[2], colors_precomp=None,
                                   scales=leaves[3], rotations=leaves[4], cov3D_precomp=None)
        return leaves, depth

    leaves, depth = render()
    assert depth.numel() == 48 * 64 and (depth > 0).any().item()
    loss = L.depth_prior_loss(depth.reshape(48, 64), prior, gt.permute(1, 2, 0), value=0.5, domin=0.1, smooth=2.0)
    loss.backward()
    g_means = leaves[0].grad
    assert torch.isfinite(g_means).all().item() and g_means.any().item()
    # by hand: the loss on a detached depth, its gradient into the rasterizer's backward
    leaves2, depth2 = render()
    assert torch.equal(depth2, depth)
    cut = depth2.detach().reshape(48, 64).clone().requires_grad_(True)
    L.depth_prior_loss(cut, prior, gt.permute(1, 2, 0), value=0.5, domin=0.1, smooth=2.0).backward()
    assert cut.grad.any().item()
    depth2.backward(cut.grad.reshape(depth2.shape))
    for a, b in zip(leaves, leaves2):
        assert torch.equal(a.grad, b.grad)
    # without depth_gradient the terms train nothing: the rasterizer drops dL/ddepth like the reference
    rast = GaussianRasterizer(raster_settings=Hh.hip_settings(c, torch.device(DEV)))
    m = c.means3D.to(DEV).clone().requires_grad_(True)
    _, _, d0 = rast(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=c.opacities.to(DEV), shs=c.shs.to(DEV),
                    colors_precomp=None, scales=c.scales.to(DEV), rotations=c.rotations.to(DEV), cov3D_precomp=None)
    loss0 = L.depth_prior_loss(d0.reshape(48, 64), prior, gt.permute(1, 2, 0), value=0.5, domin=0.1, smooth=2.0)
    assert _bits(loss0.item()) == _bits(loss.item())
    if loss0.requires_grad:
        loss0.backward()
    assert m.grad is None or not m.grad.any().item()


# ---------------------------------------------------------------- the branches no typical scene enters (DR.EDGE_SCENES)
TIED = (("tied_M", (TH + 1, TW + 1)), ("tied_M", (37, 53)), ("tied_wide", (80, 80)))


def _check_maps(s, norm=True):
    """r, o, h of the kernels bit for bit with the numpy evaluation of the header -> that evaluation"""
    r, o, h, _ = (t.cpu().numpy() for t in _L().depth_prior_maps(s.Dd, s.Pd, s.rgbd, normalise=norm))
    ev = DR.evaluate(s.D.numpy(), s.P.numpy(), s.rgb.numpy(), *W3, norm, dt=np.float32)
    for name, got, want in (("r", r, ev.r), ("o", o, ev.o), ("h", h, ev.h)):
        assert np.isfinite(want).all() and (_bits(got) == _bits(want)).all(), (name, float(np.abs(got - want).max()))
    return ev


def _check_total(label, c, mask):
    """the sum of the gradient over ``mask`` against float64, in the form of test_tied_minima_get_identical_shares"""
    exact, got, eager = c.ref.grad[mask].sum(), c.grad[mask].astype(np.float64).sum(), c.eager_grad[mask].astype(np.float64).sum()
    bound = 2 * abs(eager - exact) + FLOOR * np.abs(c.ref.grad[mask]).sum()
    print(f"{label}: kernel {got!r} eager {eager!r} float64 {exact!r}")
    assert abs(got - exact) <= bound, label


@pytest.mark.parametrize("norm", (True, False), ids=("normalised", "raw"))
@pytest.mark.parametrize("cfg", ("all", "value"))
@pytest.mark.parametrize("kind,shape", TIED, ids=lambda v: _ids(v) if isinstance(v, tuple) else v)
def test_tied_maximum_of_the_value_term(kind, shape, cfg, norm):
    """cnt_M >= 2 with both signs of e: the qM share at every l1 == M.  The tied pixels are also the tied minima and maxima
    of D and P; in tied_wide each of those ties is merged from the partials of four workgroups (scene and counts:
    test_depth_prior_cpu.py).  The gradient is one bit pattern per sign class; its total over each class, the gradient
    everywhere and the scalars are held against float64 by the measure of this file; with normalisation the shares of
    the tied extrema as well."""
    c = _case(shape, kind, cfg, norm)
    s = c.s
    neg, pos = DR.tied_pixels(kind, *shape)
    ev = _check_maps(s, norm)
    assert ev.cnt_M == len(neg) + len(pos) >= 5
    if norm:
        assert (ev.cnt_min, ev.cnt_max) == (len(neg), len(pos))
    e = (ev.r - ev.o).reshape(-1)
    assert (e[neg] == -ev.M).all() and (e[pos] == ev.M).all()
    _check_scalars(f"{shape} {kind} {cfg} norm={norm}", c.out, c.eager_out, c.ref.out)
    print(f"gradient {shape} {kind} {cfg} norm={norm}: kernel {c.err:.3e} eager {c.eager_err:.3e}")
    assert np.isfinite(c.grad).all() and c.err <= 2 * c.eager_err + FLOOR
    g = c.grad.reshape(-1)
    for name, group in (("e = -M", neg), ("e = +M", pos)):
        assert (_bits(g[group]) == _bits(g[group])[0]).all() and g[group[0]] != 0, name
        mask = np.zeros(g.size, bool)
        mask[group] = True
        _check_total(f"tied total {shape} {kind} {cfg} norm={norm} {name}", c, mask.reshape(shape))
    if norm:
        # what the normalisation adds on top of G / range at the tied extrema: the equal shares
        ev64 = DR.evaluate(s.D.numpy(), s.P.numpy(), s.rgb.numpy(), *CONFIGS[cfg], True, dt=np.float64)
        direct = (ev64.G / 4.00000001).reshape(-1)
        for group, share in ((neg, ev64.share_min), (pos, ev64.share_max)):
            exact = c.ref.grad.reshape(-1)[group[0]] - direct[group[0]]
            assert abs(exact - share) <= 1e-11 * max(abs(c.ref.grad.reshape(-1)[group[0]]), abs(share))
            got, eager = float(g[group[0]]) - direct[group[0]], float(c.eager_grad.reshape(-1)[group[0]]) - direct[group[0]]
            assert abs(got - exact) <= 2 * abs(eager - exact) + FLOOR * abs(c.ref.grad.reshape(-1)[group[0]])


def test_clamp_gates_of_the_distribution_term_pixel_by_pixel():
    """The per-pixel gates |r| <= 1e6 and t t <= 1e6 (scenes and memberships: test_depth_prior_cpu.py): beyond the bound the
    gradient is exactly 0, at the bound and elsewhere it is float64 autograd's (torch.clamp passes it at the bound)."""
    D, P = DR.clamp_gate_scene()
    w = CONFIGS["domin"]
    ref = DR.autograd64(D, P, torch.zeros(5, 5, 3), *w, False)
    eager_out, eager_grad = _eager(D.to(DEV), P.to(DEV), torch.zeros(5, 5, 3, device=DEV), w, False)
    out, grad = _run(D.to(DEV), P.to(DEV), None, w, False)
    beyond = np.abs(D.numpy()) > 1e6
    assert beyond.sum() == 3 and not grad[beyond].any() and grad[~beyond].all()
    assert grad[2, 2] != 0 and grad[3, 1] != 0
    _check_scalars("clamp gates 5x5", out, eager_out, ref.out)
    err, eager_err = Hh.max_err_over_scale(grad, ref.grad), Hh.max_err_over_scale(eager_grad, ref.grad)
    print(f"gradient clamp gates 5x5: kernel {err:.3e} eager {eager_err:.3e}")
    assert err <= 2 * eager_err + FLOOR
    # S == 1e6 exactly: the sum gate is open, the pixel's own gate is closed
    one_D, one_P = torch.full((1, 1), 2000.0, device=DEV), torch.zeros(1, 1, device=DEV)
    out, grad = _run(one_D, one_P, None, w, False)
    want = np.sqrt(1e6 + 1e-6) + 4 * np.sqrt(float(np.float32(1e-6)) ** 2 + 1e-6)
    assert abs(float(out[2]) - want) <= _unit(want) and out[1] == 0 and out[3] == 0
    assert grad.shape == (1, 1) and grad[0, 0] == 0


@pytest.mark.parametrize("kind", ("noise", "rendered"))
@pytest.mark.parametrize("shape", ((1, 1), (1, 40), (40, 1), (2, 40)), ids=_ids)
def test_thin_shapes_without_the_value_term(shape, kind):
    """H = 1 or W = 1 with smoothness + distribution: in the border form of A2 both gy == 0 and gy == H - 1 hold.  (The
    maps call forms h, a value-term quantity, so it exists from 2 x 2 on: checked at (2, 40).)"""
    c = _case(shape, kind, "ds")
    _check_scalars(f"{shape} {kind} thin", c.out, c.eager_out, c.ref.out)
    assert c.out[1] == 0 and c.grad.shape == shape and np.isfinite(c.grad).all()
    print(f"gradient {shape} {kind} thin: kernel {c.err:.3e} eager {c.eager_err:.3e}")
    if np.abs(c.ref.grad).max() > 0:
        assert c.err <= 2 * c.eager_err + FLOOR
    else:
        assert not c.grad.any()
    if min(shape) >= 2:
        _check_maps(c.s)
    else:
        with pytest.raises(ValueError, match="at least 2"):
            _run(c.s.Dd, c.s.Pd, c.s.rgbd)


def test_grid_stride_of_the_tiled_kernels():
    """(16 * 16385, 2): 16385 tiles of two pixels' width for at most 16384 workgroups, so workgroup 0 walks a second tile.
    All three terms at once (float64 autograd through unfold takes about a second at this size)."""
    shape = (16 * 16385, 2)
    c = _case(shape, "noise")
    _check_maps(c.s)
    _check_scalars(f"{shape} noise", c.out, c.eager_out, c.ref.out)
    print(f"gradient {shape}: kernel {c.err:.3e} eager {c.eager_err:.3e}")
    assert np.isfinite(c.grad).all() and c.err <= 2 * c.eager_err + FLOOR
    last = slice(16 * 16384, None)                      # the wrapped tile, on its own
    assert Hh.max_err_over_scale(c.grad[last], c.ref.grad[last]) <= 2 * Hh.max_err_over_scale(c.eager_grad[last], c.ref.grad[last]) + FLOOR


@pytest.mark.parametrize("shape", ((TH + 1, TW + 1), (37, 53)), ids=_ids)
def test_near_flat_depth(shape):
    """max - min of D is three fp32 units of D: the 1e-8 of the range is 1.4 % of it."""
    for cfg, norm in (("all", True), ("value", True), ("smooth", True)):
        c = _case(shape, "near_flat", cfg, norm)
        _check_scalars(f"{shape} near_flat {cfg}", c.out, c.eager_out, c.ref.out)
        print(f"gradient {shape} near_flat {cfg}: kernel {c.err:.3e} eager {c.eager_err:.3e}")
        assert np.isfinite(c.grad).all() and c.err <= 2 * c.eager_err + FLOOR
    _check_maps(_scene(shape, "near_flat"))


@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_depth_gives_nan_scalars_and_leaves_no_state(bad):
    """The header's deviation 1: no asserts, a NaN (or inf) pixel of D gives NaN scalars and the call returns.  Nothing
    survives it: the same clean call before and after is bit-equal.  (Nothing is said about the gradient.)"""
    s = _scene((37, 53), "noise")
    before = _run(s.Dd, s.Pd, s.rgbd)
    D = s.Dd.clone()
    D[11, 17] = bad
    out, grad = _run(D, s.Pd, s.rgbd)
    torch.cuda.synchronize()
    assert np.isnan(out).all(), out
    after = _run(s.Dd, s.Pd, s.rgbd)
    assert np.isfinite(after[0]).all()
    assert (_bits(before[0]) == _bits(after[0])).all() and (_bits(before[1]) == _bits(after[1])).all()
