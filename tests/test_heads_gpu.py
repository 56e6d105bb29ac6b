"""The anchor heads on the GPU (include/bloomscene_heads.h, bloomscene_amd/heads.py) against tests/heads_reference.py:
the pre-activations and scale_rot bit for bit with the numpy evaluation of the header's chains, everything that holds a
transcendental or a sum over rows against float64 autograd of the restatement (with the gate of the fp32 chain, see the
reference), with the fp32 eager lines on the same GPU as the measure of what fp32 can do:

    kernel error <= 2 x eager error + 2^-23        (helpers.max_err_over_scale, pooled over the small n per (F, K))

Rows, relative to the kernels' tiles (64 rows a workgroup in the forward and the row pass, ranges of 256 rows in the weight
sums): 1, 2, 63, 64, 65, 127, 255, 256, 257; (50, 10) once at 4099 rows, 17 ranges.  Every case is evaluated once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import heads_reference as HR
import helpers as Hh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((50, 10), (4, 1), (7, 3), (64, 16))
SMALL_N = (1, 2, 63, 64, 65, 127, 255, 256, 257)
BIG = (50, 10, 4099)
FLOOR = 2.0 ** -23


def _H():
    import bloomscene_amd.heads as H
    return H


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _leaves(s, grad=True, weights_grad=True):
    d = lambda t, g: t.to(DEV).clone().requires_grad_(g)
    return SimpleNamespace(feat=d(s.feat, grad), anchor=d(s.anchor, grad), cam=s.cam.to(DEV),
                           mask=None if s.mask is None else d(s.mask, grad),
                           weights=[d(w, grad and weights_grad) for w in s.weights])


def _grads(l):
    g = lambda t: None if t is None or t.grad is None else t.grad.detach().cpu().numpy()
    return SimpleNamespace(d_feat=g(l.feat), d_anchor=g(l.anchor), d_mask=g(l.mask), d_weights=[g(w) for w in l.weights])


def _kernel(s, heads=(0, 1, 2), **kw):
    """forward + backward of the fused call -> outputs (numpy), gradients"""
    l = _leaves(s, **kw)
    outs = _H().anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, s.K, offset_mask=l.mask)
    ups = [u.to(DEV) for u in s.ups]
    terms = [(outs[0], ups[0]), (outs[2], ups[2]), (outs[1], ups[1])]
    sum((terms[h][0] * terms[h][1]).sum() for h in heads).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], _grads(l)


def _eager(s, gate, heads=(0, 1, 2)):
    l = _leaves(s)
    outs = HR.restatement(l.feat, l.anchor, l.cam, l.weights, s.K, l.mask, torch.as_tensor(gate, device=DEV))
    ups = [u.to(DEV) for u in s.ups]
    terms = [(outs[0], ups[0]), (outs[2], ups[2]), (outs[1], ups[1])]
    sum((terms[h][0] * terms[h][1]).sum() for h in heads).backward()
    return [o.detach().cpu().numpy() for o in outs], _grads(l)


@functools.lru_cache(maxsize=None)
def _case(F, K, n):
    """the numpy chains, float64 autograd, the eager fp32 lines and the kernels for one call, computed once"""
    s = HR.scene(n, F, K, seed=n)
    c = SimpleNamespace(s=s)
    c.np = HR.forward_np(s.feat.numpy(), s.anchor.numpy(), s.cam.numpy(), [w.numpy() for w in s.weights], K)
    c.ref = HR.autograd64(s.feat, s.anchor, s.cam, s.weights, K, s.mask, s.ups, c.np.gate)
    l = _leaves(s, grad=False)
    c.maps = [t.cpu().numpy() for t in _H().anchor_heads_maps(l.feat, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)]
    c.out, c.grad = _kernel(s)
    c.eager_out, c.eager_grad = _eager(s, c.np.gate.astype(np.float32))
    return c


def _cases(F, K):
    return [_case(F, K, n) for n in SMALL_N]


def _rule(label, got, eager, ref):
    err, eager_err = Hh.max_err_over_scale(got, ref), Hh.max_err_over_scale(eager, ref)
    print(f"[heads] {label:36s} kernel {err:.3e} eager {eager_err:.3e}")
    assert np.isfinite(got).all(), label
    assert err <= 2 * eager_err + FLOOR, (label, err, eager_err)


def _gradient_rule(label, cases):
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])
    for name in ("d_feat", "d_anchor", "d_mask"):
        _rule(f"{label} {name}", cat(getattr(c.grad, name) for c in cases), cat(getattr(c.eager_grad, name) for c in cases),
              cat(getattr(c.ref, name) for c in cases))
    for i, name in enumerate(_H().WEIGHT_NAMES):
        _rule(f"{label} d {name}", cat(c.grad.d_weights[i] for c in cases), cat(c.eager_grad.d_weights[i] for c in cases),
              cat(c.ref.d_weights[i] for c in cases))


@pytest.mark.parametrize("F,K", SHAPES)
def test_pre_activations_and_scale_rot_are_the_headers_chains_bit_for_bit(F, K):
    for c in _cases(F, K) + ([_case(*BIG)] if (F, K) == BIG[:2] else []):
        n = c.s.n
        opacity, color, scale_rot, pre1, pre2 = c.maps
        assert pre1.shape == (n, 3 * F) and pre2.shape == (n, 11 * K)
        assert (_bits(pre1) == _bits(c.np.pre1)).all(), (n, "pre1")
        assert (_bits(pre2) == _bits(c.np.pre2)).all(), (n, "pre2")
        assert (_bits(scale_rot) == _bits(c.np.pre2[:, K:8 * K].reshape(n * K, 7))).all(), (n, "scale_rot")
        for got, again in zip(c.out, c.maps[:3]):      # the differentiable call writes the same outputs
            assert (_bits(got) == _bits(again)).all()
        zeros = c.s.mask.reshape(-1).numpy() == 0
        assert zeros.any() or n < 3
        assert (_bits(opacity.reshape(-1)[zeros]) & 0x7fffffff == 0).all()
        assert (opacity.reshape(-1)[~zeros] != 0).all()
        assert opacity.shape == (n * K, 1) and color.shape == (n * K, 3) and scale_rot.shape == (n * K, 7)


@pytest.mark.parametrize("F,K", SHAPES)
def test_activated_outputs_against_float64(F, K):
    cases = _cases(F, K)
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])
    _rule(f"({F}, {K}) neural_opacity", cat(c.out[0] for c in cases), cat(c.eager_out[0] for c in cases), cat(c.ref.opacity for c in cases))
    _rule(f"({F}, {K}) color", cat(c.out[1] for c in cases), cat(c.eager_out[1] for c in cases), cat(c.ref.color for c in cases))


@pytest.mark.parametrize("F,K", SHAPES)
def test_gradients_against_float64_autograd(F, K):
    _gradient_rule(f"({F}, {K})", _cases(F, K))


def test_gradients_where_several_ranges_meet():
    c = _case(*BIG)
    _gradient_rule("(50, 10) n = 4099", [c])
    _rule("(50, 10) n = 4099 neural_opacity", c.out[0], c.eager_out[0], c.ref.opacity)
    _rule("(50, 10) n = 4099 color", c.out[1], c.eager_out[1], c.ref.color)


def test_rows_are_pure_functions_of_their_row():
    F, K, n = 50, 10, 257
    c = _case(F, K, n)
    s = c.s
    for a, b in ((60, 130), (256, 257), (0, 64)):
        sub = SimpleNamespace(n=b - a, F=F, K=K, feat=s.feat[a:b], anchor=s.anchor[a:b], cam=s.cam, weights=s.weights,
                              mask=s.mask[a:b], ups=tuple(u[a * K:b * K] for u in s.ups))
        out, grad = _kernel(sub)
        for got, full in zip(out, c.out):
            assert (_bits(got) == _bits(full[a * K:b * K])).all()
        assert (_bits(grad.d_feat) == _bits(c.grad.d_feat[a:b])).all()
        assert (_bits(grad.d_anchor) == _bits(c.grad.d_anchor[a:b])).all()
        assert (_bits(grad.d_mask) == _bits(c.grad.d_mask[a:b])).all()
    # feat as a view with a row stride of 2 F: the bits of the contiguous copy, and a dense gradient to the view's base
    wide = torch.randn(n, 2 * F)
    wide[:, :F] = s.feat
    base = wide.to(DEV).requires_grad_(True)
    l = _leaves(s)
    view = base[:, :F]
    assert view.stride() == (2 * F, 1)
    outs = _H().anchor_heads_tensors(view, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)
    sum((o * u.to(DEV)).sum() for o, u in zip(outs, s.ups)).backward()
    for got, full in zip(outs, c.out):
        assert (_bits(got) == _bits(full)).all()
    assert (_bits(base.grad[:, :F]) == _bits(c.grad.d_feat)).all() and not base.grad[:, F:].any()
    for got, full in zip(l.weights, c.grad.d_weights):
        assert (_bits(got.grad) == _bits(full)).all()


def test_two_runs_give_the_same_bits():
    c = _case(*BIG)
    out, grad = _kernel(c.s)
    for a, b in zip(out, c.out):
        assert (_bits(a) == _bits(b)).all()
    for name in ("d_feat", "d_anchor", "d_mask"):
        assert (_bits(getattr(grad, name)) == _bits(getattr(c.grad, name))).all(), name
    for name, a, b in zip(_H().WEIGHT_NAMES, grad.d_weights, c.grad.d_weights):
        assert (_bits(a) == _bits(b)).all(), name


def test_only_the_heads_used_downstream_contribute():
    F, K, n = 50, 10, 257
    c = _case(F, K, n)
    s = c.s
    out, grad = _kernel(s, heads=(2,))                          # color alone: the other upstreams are None
    ref = HR.autograd64(s.feat, s.anchor, s.cam, s.weights, K, s.mask, s.ups, c.np.gate, heads=(2,))
    _, eager = _eager(s, c.np.gate.astype(np.float32), heads=(2,))
    for i in range(8):
        assert grad.d_weights[i] is not None and not grad.d_weights[i].any(), _H().WEIGHT_NAMES[i]
    assert not grad.d_mask.any()
    _rule("color only d_feat", grad.d_feat, eager.d_feat, ref.d_feat)
    _rule("color only d_anchor", grad.d_anchor, eager.d_anchor, ref.d_anchor)
    for i in range(8, 12):
        _rule(f"color only d {_H().WEIGHT_NAMES[i]}", grad.d_weights[i], eager.d_weights[i], ref.d_weights[i])
    # frozen weights: only feat, anchor (and the mask) receive a gradient -- the same bits, without the sums
    out, frozen = _kernel(s, weights_grad=False)
    assert all(g is None for g in frozen.d_weights)
    assert (_bits(frozen.d_feat) == _bits(c.grad.d_feat)).all() and (_bits(frozen.d_anchor) == _bits(c.grad.d_anchor)).all()
    assert (_bits(frozen.d_mask) == _bits(c.grad.d_mask)).all()


def test_no_grad_allocates_the_outputs_only():
    F, K, n = BIG
    s = _case(F, K, n).s
    l = _leaves(s, grad=False)
    H = _H()
    with torch.no_grad():
        H.anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)      # (loads everything)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs = H.anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    outputs = sum(o.numel() * 4 for o in outs)
    assert outputs == n * K * 11 * 4
    assert peak <= outputs + 3 * 512, (peak, outputs)          # (the allocator's rounding per tensor)
    assert peak < outputs + n * 3 * F * 4


def test_no_rows():
    H = _H()
    F, K = 50, 10
    s = HR.scene(0, F, K)
    l = _leaves(s)
    outs = H.anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)
    assert [tuple(o.shape) for o in outs] == [(0, 1), (0, 3), (0, 7)]
    sum(o.sum() for o in outs).backward()
    assert l.feat.grad.shape == (0, F) and l.anchor.grad.shape == (0, 3)
    for w in l.weights:
        assert w.grad is not None and w.grad.shape == w.shape and not w.grad.any()
    maps = H.anchor_heads_maps(l.feat.detach(), l.anchor.detach(), l.cam, [w.detach() for w in l.weights], K)
    assert maps[3].shape == (0, 3 * F) and maps[4].shape == (0, 11 * K)


def test_double_backward_is_refused():
    s = HR.scene(5, 7, 3)
    l = _leaves(s)
    out = _H().anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, 3, offset_mask=l.mask)[2]
    g, = torch.autograd.grad(out.sum(), l.feat, create_graph=True)
    with pytest.raises(RuntimeError):         # (no graph behind the gradient: it is never treated as a constant silently)
        g.sum().backward()


@pytest.mark.parametrize("F,K", ((50, 10), (64, 16)))
def test_forward_and_backward_replay_from_a_graph_without_a_host_wait(F, K):
    """Forward and backward captured with torch.cuda.graph after one warm-up call (capture raises on any host wait), on
    one stream, and replayed on new input values: bit-equal to the direct call.  (64, 16): the row pass asks for more
    than 64 KiB of LDS."""
    H = _H()
    n = 257
    s, s2 = HR.scene(n, F, K, seed=31), HR.scene(n, F, K, seed=32)
    l = _leaves(s)
    ups = [u.to(DEV) for u in s.ups]
    leaves = [l.feat, l.anchor, l.mask] + l.weights

    def step():
        outs = H.anchor_heads_tensors(l.feat, l.anchor, l.cam, l.weights, K, offset_mask=l.mask)
        grads = torch.autograd.grad(sum((o * u).sum() for o, u in zip(outs, ups)), leaves)
        return tuple(outs) + tuple(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                           # the warm-up: loads the library
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    l2 = _leaves(s2)
    with torch.no_grad():                                # new values in the captured tensors
        for dst, src in zip(leaves + ups + [l.cam], [l2.feat, l2.anchor, l2.mask] + l2.weights + [u.to(DEV) for u in s2.ups]
                            + [torch.tensor([-0.5, 0.1, 3.0], device=DEV)]):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    direct = step()
    torch.cuda.synchronize()
    assert not torch.equal(replayed[0], torch.as_tensor(_case(F, K, n).out[0], device=DEV))
    for a, b in zip(replayed, direct):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_training_view_with_the_fused_heads():
    """views.training_view(heads=AnchorHeads(...)) on a small synthetic scene, then a backward: every MLP weight
    receives a finite, non-zero gradient, and render, radii, depth are bit for bit those of the same call with heads that
    return the outputs the bit test pins (the kernels' own, evaluated outside)."""
    from bloomscene_amd import views
    from bloomscene_amd.synthetic import anchor_scene, upstream_grads
    H = _H()
    dev = torch.device(DEV)
    N, K, F, W, Hh_ = 3000, 10, 50, 160, 96
    sc = anchor_scene(N, K, W, Hh_, seed=5)
    g = torch.Generator().manual_seed(9)
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g)).to(dev)
    torch.manual_seed(3)
    mlps = [nn.Sequential(nn.Linear(F + 4, F), nn.ReLU(True), nn.Linear(F, o * K), *([act()] if act else [])).to(dev)
            for o, act in zip((1, 7, 3), (nn.Tanh, None, nn.Sigmoid))]
    with torch.no_grad():
        mlps[0][2].bias.add_(1.0)                        # (most offsets opaque enough to be selected)
    feat = torch.randn(N, F, generator=g).to(dev).requires_grad_(True)
    mask_full = (torch.rand(N, K, 1, generator=g) < 0.8).float().to(dev)
    cam = sc.camera.to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    gC, gD = (t.to(dev) for t in upstream_grads(W, Hh_, seed=2))
    anchor, scaling, offsets = (t.to(dev).clone().requires_grad_(True) for t in (sc.anchor, sc.grid_scaling, sc.grid_offsets))
    heads = H.AnchorHeads(*mlps, feat=feat, anchor=anchor, camera_center=cam.camera_center.to(dev), offset_mask=mask_full)
    res = views.training_view(cam, anchor, scaling, rot, offsets, heads, bg)
    assert int(res["visible_idx"].numel()) > 64 and bool(res["selection_mask"].any())
    torch.autograd.backward((res["render"], res["depth"]), (gC, gD))
    for mlp in mlps:
        for p in mlp.parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any())
    assert bool(torch.isfinite(feat.grad).all()) and bool(feat.grad.any())

    def pinned(idx):
        with torch.no_grad():
            return H.anchor_heads_maps(feat.detach().index_select(0, idx), anchor.detach().index_select(0, idx),
                                       cam.camera_center.to(dev), H.head_weights(*mlps), K,
                                       offset_mask=mask_full.index_select(0, idx))[:3]
    with torch.no_grad():
        ref = views.training_view(cam, anchor.detach(), scaling.detach(), rot, offsets.detach(), pinned, bg)
    for k in ("render", "radii", "depth"):
        assert torch.equal(res[k], ref[k]), k
