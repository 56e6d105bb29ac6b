"""The kernels of bloomscene_amd/csrc/anchors.hip on the branches tests/test_anchors_gpu.py never enters, against
tests/anchor_expand_reference.py (which tests/test_anchor_expand_reference_cpu.py holds against float64 autograd and
whose inputs it shows to discriminate).

- scan rounds: k_anchor_scan with 8192 counts (one full round), 8193 (a second round of one count) and 16385 (a third),
  its carry and its partial last round; the same scan behind bsr_visible_filter_indices at 8194 counts;
- awkward K: K = 2, 85, 86, 128, 129, 255 (A = 128, 3, 2, 2, 1, 1 anchors per workgroup, up to 127 dead lanes), the
  per-anchor sums BIT for bit in slot order; K = 257 and N * K = 2^31 are refused;
- the clamped norm: `len <= 1e-12` in the backward with a non-NULL dL_drot;
- every upstream-NULL branch of the backward, and every `extra[]` addition of bsr_anchor_render_backward;
- the fused forward's buffer-size guess when it is short (second allocation) and far too large (layout follows S);
- BSR_FLAG_NO_READBACK with every candidate selected and with none.

Gradients that are one rounding per operation are compared bit for bit.  Those through the sigmoid and the norm are held
to the siblings' rule of tests/test_adam_gpu.py, measured against float64: the kernel's distance is at most twice eager
fp32 torch's on the same device plus 2^-23 of the scale, per row class and column group; where no eager run is made
(awkward K, the two-round shape), to an a-priori bound from the formats (see _apriori)."""
import math

import numpy as np
import pytest
import torch

import anchor_expand_reference as AE
from oracle import anchors as OA

pytestmark = pytest.mark.gpu

NAMES = AE.UPSTREAMS
IN_NAMES = AE.IN_NAMES
U24 = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_forward(inp, out=None):
    """The rule of tests/test_anchors_gpu.py: mask, xyz, color, opacity bit-exact; scaling and rot to 1e-6 relative."""
    from bloomscene_amd.neural_gaussians import expand_anchors
    ref = OA.expand_anchors_reference(*inp)
    if out is None:
        out = expand_anchors(*[t.to(_dev()) for t in inp])
    assert out[5].dtype == torch.bool and torch.equal(out[5].cpu(), ref[5])
    for name, a, b in zip(NAMES, out[:5], ref[:5]):
        a = a.detach().cpu()
        assert a.shape == b.shape and a.dtype == torch.float32, name
        if name in ("xyz", "color", "opacity"):
            assert _bits(a, b), name
        else:
            err = (a.double() - b.double()).abs()
            assert bool((err <= 1e-6 * b.double().abs() + 1e-30).all()), (name, float((err / (b.abs() + 1e-30)).max()))
    return ref, out


def _backward(fn, inp, up, dev):
    """Gradients (numpy, one per input) of `fn` for the upstreams that are not None; none at all: backward through an
    output multiplied by zero."""
    leaves = [t.detach().to(dev).requires_grad_(True) for t in inp]
    out = fn(*leaves)
    idx = [i for i, n in enumerate(NAMES) if up[n] is not None]
    if idx:
        torch.autograd.backward([out[i] for i in idx], [up[NAMES[i]].to(dev) for i in idx])
    else:
        (out[0].sum() * 0.0).backward()
    return [np.zeros(tuple(l.shape), np.float32) if l.grad is None else l.grad.detach().cpu().numpy() for l in leaves], out


def _assert_exact_set(got, want, N, K, sel):
    """d_anchor, d_gs[:, 0:3], d_offsets, d_color, d_neural_opacity: the restatement's bits; unselected rows zero."""
    d_anchor, d_gs, d_off, d_nop, d_col, d_sr = got
    assert AE.bits_equal(d_anchor, want["d_anchor"])
    assert AE.bits_equal(d_gs[:, :3], want["d_gs_xyz"])
    assert AE.bits_equal(d_off.reshape(N * K, 3), want["d_offsets"])
    assert AE.bits_equal(d_col.reshape(N * K, 3), want["d_color"])
    assert AE.bits_equal(d_nop.reshape(-1), want["d_neural_opacity"])
    for g in (d_off, d_nop, d_col, d_sr):
        assert not g.reshape(N * K, -1)[~sel].any()


def _rule(label, kernel, eager, ref):
    """tests/test_adam_gpu.py: the kernel is at most twice as far from float64 as eager torch, plus 2^-23 of the scale."""
    d_k, d_e, scale = (float(np.abs(kernel - ref).max()), float(np.abs(eager - ref).max()), float(np.abs(ref).max()))
    print(f"{label}: kernel {d_k:.3e}, eager torch {d_e:.3e}, scale {scale:.3e}")
    assert np.isfinite(kernel).all(), label
    assert d_k <= 2 * d_e + 2.0 ** -23 * scale, (label, d_k, d_e, scale)
    return 2 * d_e + 2.0 ** -23 * scale


def _apriori(got, inp, up, want, N, K):
    """d_gs[:, 3:6] and d_sr against the float64 restatement with bounds from the fp32 format alone.  u = 2^-24.
    sigmoid s = 1 / (1 + exp(-x)): bsr_expf within 1 ulp = 2 u, one addition, one division: 4 u relative.
    d_sr[:, 0:3] = fl(g gs) * fl(s fl(1 - s)): 1 - s inherits 4 u s ABSOLUTE (not relative: s may be near 1), so
    s (1 - s) is within u (6 s (1 - s) + 4 s^2), and with the two outer products the value within 8 u |g gs| s.
    d_gs[:, 3:6] = sum over K slots of fl(g * s): each term 5 u, the K additions in order (K - 1) u of the sum of
    magnitudes: <= (K + 4) u sum |g s|.  d_sr[:, 3:7] normal branch (g - r (r.g)) / |v|: |v| 3 u, 1 / |v| 4 u, r 5 u, the
    dot product of four 9 u of |r|.|g|, r_c * dot 15 u of it, the subtraction and the last product 6 u of their operand:
    every component within 24 u (|g_c| + |r|.|g|) / |v|; clamped branch g / 1e-12f: the division's u plus the 4e-9
    between 1e-12f and 1e-12."""
    d_gs, d_sr = got[1].astype(np.float64), got[5].astype(np.float64).reshape(N * K, 7)
    sel = inp[3].numpy().reshape(-1) > 0
    sr = inp[5].numpy().astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-sr[:, :3]))
    gsc = AE._scatter(None if up["scaling"] is None else up["scaling"].numpy(), sel, 3, np.float64)
    mag = np.abs(gsc * s).reshape(N, K, 3).sum(axis=1)
    assert (np.abs(d_gs[:, 3:] - want["d_gs_scale"]) <= (K + 4) * U24 * mag).all()
    gs_rep = np.repeat(inp[1].numpy().astype(np.float64)[:, 3:], K, axis=0)
    assert (np.abs(d_sr[:, :3] - want["d_sr"][:, :3]) <= 8 * U24 * np.abs(gsc * gs_rep) * s).all()
    g = AE._scatter(None if up["rot"] is None else up["rot"].numpy(), sel, 4, np.float64)
    v = sr[:, 3:7]
    length = np.sqrt((v * v).sum(axis=1, keepdims=True))
    normal = length > AE.EPS
    safe = np.where(normal, length, 1.0)
    bound = np.where(normal, 24 * U24 * (np.abs(g) + (np.abs(v / safe) * np.abs(g)).sum(axis=1, keepdims=True)) / safe,
                     2 * U24 * np.abs(g) / AE.EPS)
    assert (np.abs(d_sr[:, 3:] - want["d_sr"][:, 3:]) <= bound).all()


# ------------------------------------------------------------------------------------------------ scan rounds
@pytest.mark.parametrize("N,K", AE.SCAN_SHAPES, ids=lambda v: str(v))
def test_scan_rounds_forward(N, K):
    """8192 workgroup counts: one full round of k_anchor_scan; 8193: a second round whose one count needs s_carry; 16385:
    a third.  The selection density varies by region and 300 workgroups across the round boundary select nothing, so a
    lost or doubled carry, or a wrong tail of the partial round, moves rows (shown on the CPU)."""
    inp = AE.scan_inputs(N, K)
    assert AE.workgroups(N, K) in (8192, 8193, 16385)
    ref, out = _check_forward(inp)
    assert 0 < out[0].shape[0] < N * K


def test_scan_second_round_backward_against_the_restatement():
    """(8193, 129): the backward reads wg_base of the second round; K = 129 leaves 127 of 256 lanes dead and one anchor
    per workgroup.  All five upstreams; the exact set bit for bit, the rest within the a-priori bounds."""
    from bloomscene_amd.neural_gaussians import expand_anchors
    N, K = AE.SCAN_SHAPES[1]
    inp = AE.scan_inputs(N, K)
    sel = inp[3].numpy().reshape(-1) > 0
    up = AE.upstreams(int(sel.sum()), seed=3)
    got, _ = _backward(expand_anchors, inp, up, _dev())
    want = AE.restate(inp, up, K)
    _assert_exact_set(got, want, N, K, sel)
    _apriori(got, inp, up, want, N, K)


def test_visible_filter_indices_across_a_scan_round():
    """bsr_visible_filter_indices at P = 8192 * 256 + 257: 8194 workgroup counts, a second round of two (the last with
    one point).  Points in front of and behind the camera alternate in blocks of irregular length."""
    from bloomscene_amd import GaussianRasterizer, cameras, views
    dev = _dev()
    P = AE.VISIBLE_P
    front = torch.from_numpy(AE.visible_pattern())
    g = torch.Generator().manual_seed(6)
    xyz = torch.rand(P, 3, generator=g) * torch.tensor([2.0, 1.0, 2.0]) + torch.tensor([-1.0, -0.5, 4.0])
    xyz[:, 2] = torch.where(front, xyz[:, 2], -xyz[:, 2])
    scales = torch.full((P, 3), 0.02)
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(P, 4).contiguous()
    cam = cameras.identity_camera(128, 80, math.radians(60)).to(dev)
    rast = GaussianRasterizer(views.make_settings(cam, torch.zeros(3, device=dev), 1))
    radii, idx = rast.visible_filter_indices(xyz.to(dev), scales.to(dev), rot.to(dev))
    want = (radii > 0).nonzero().squeeze(1)
    assert idx.dtype == torch.int64 and torch.equal(idx, want)
    vis = (radii > 0).cpu()
    assert not vis[~front].any() and 0.3 * P < int(vis.sum()) < 0.7 * P
    assert bool(vis[8192 * 256:].any())      # the second round writes indices


# ------------------------------------------------------------------------------------------------ awkward K
@pytest.mark.parametrize("K", AE.AWKWARD_K)
def test_awkward_K_forward_and_backward(K):
    """A = 256 // K drops from 3 to 2 between K = 85 and 86 and from 2 to 1 between 128 and 129; N = 3 A + 1 leaves the
    last workgroup with one anchor.  The per-anchor sums must be the slot-order sums, bit for bit."""
    from bloomscene_amd.neural_gaussians import expand_anchors
    inp = AE.awkward_inputs(K)
    N = inp[0].shape[0]
    assert N == 3 * (256 // K) + 1 and AE.workgroups(N, K) == 4
    sel = inp[3].numpy().reshape(-1) > 0
    up = AE.upstreams(int(sel.sum()), seed=K)
    got, out = _backward(expand_anchors, inp, up, _dev())
    _check_forward(inp, out)
    want = AE.restate(inp, up, K)
    _assert_exact_set(got, want, N, K, sel)
    _apriori(got, inp, up, want, N, K)


def test_out_of_range_shapes_are_refused():
    from bloomscene_amd import _capi
    from bloomscene_amd.neural_gaussians import expand_anchors
    dev = _dev()
    inp = OA.synthetic_anchor_inputs(2, 257, seed=0)
    with pytest.raises(RuntimeError):
        expand_anchors(*[t.to(dev) for t in inp])
    lib = _capi.lib()
    assert lib.bsr_anchor_scratch_bytes(2 ** 23, 256) == 0          # N * K = 2^31
    assert lib.bsr_anchor_scratch_bytes(2 ** 23 - 1, 256) > 0
    assert lib.bsr_anchor_scratch_bytes(2, 257) == 0 and lib.bsr_anchor_scratch_bytes(2, 0) == 0


# ------------------------------------------------------------------------------------------------ clamped norm
def _ref_autograd(inp, up):
    leaves = [t.double().requires_grad_(True) for t in inp]
    out = OA.expand_anchors_reference(*leaves)
    torch.autograd.backward(list(out[:5]), [up[n].double() for n in NAMES])
    return [l.grad.numpy() for l in leaves]


def test_clamped_norm_forward_and_backward():
    """|v| = 0, 3e-13 and 2e-13 enter `len <= 1e-12` of the backward with dL_drot present; 2e-12 and 2e-7 sit on the
    other side.  Forward: the clamped rows are v / 1e-12.  Backward: d_sr and d_gs[:, 3:6] by the siblings' rule against
    float64 autograd, per row class and column group (finer, per kind of row, as well: that implies the coarser)."""
    from bloomscene_amd.neural_gaussians import expand_anchors
    dev = _dev()
    inp, kind = AE.clamped_inputs()
    N, K = 40, 10
    up = AE.upstreams(N * K, seed=8)
    got, out = _backward(expand_anchors, inp, up, dev)
    eager, _ = _backward(OA.expand_anchors_reference, inp, up, dev)
    _check_forward(inp, out)
    clamped = torch.tensor(AE.CLAMPED)[kind]
    rot, v = out[4].detach().cpu().double(), inp[5][:, 3:7].double()
    assert bool(((rot[clamped] - v[clamped] / 1e-12).abs() <= 1e-6 * (v[clamped] / 1e-12).abs()).all())
    assert not rot[kind == 0].any() and bool((rot[kind == 1][:, 0] - 0.3).abs().max() < 1e-6)
    ref = _ref_autograd(inp, up)
    sel = np.ones(N * K, bool)
    _assert_exact_set(got, AE.restate(inp, up, K), N, K, sel)
    _rule("d_gs[:, 3:6]", got[1][:, 3:], eager[1][:, 3:], ref[1][:, 3:])
    clamped = clamped.numpy()
    tol = {}
    for rows, rname in ((clamped, "clamped"), (~clamped, "normal")):
        for cols, cname in ((slice(0, 3), "0:3"), (slice(3, 7), "3:7")):
            tol[rname, cname] = _rule(f"d_sr[{rname} rows, {cname}]", got[5][rows, cols], eager[5][rows, cols],
                                      ref[5][rows, cols])
    # the clamped rows' tolerance cannot hide the normal-branch formula (tests/test_anchor_expand_reference_cpu.py)
    assert tol["clamped", "3:7"] < AE.CLAMP_MARGIN * float(np.abs(ref[5][clamped, 3:]).max())
    for k, name in enumerate(AE.CLAMP_KINDS):
        rows = (kind == k).numpy()
        _rule(f"d_sr[{name} rows, 3:7]", got[5][rows, 3:], eager[5][rows, 3:], ref[5][rows, 3:])


# ------------------------------------------------------------------------------------------------ upstream subsets
@pytest.mark.parametrize("names", AE.SUBSETS, ids=lambda n: "+".join(n) or "none")
def test_backward_with_a_subset_of_the_upstreams(names):
    """Each of the five upstream-NULL branches of k_anchor_expand_bwd on its own.  A backward of the same shape with
    other values runs first, so the allocator hands the second run buffers that hold those: every gradient must be
    fully overwritten, unselected rows exactly zero."""
    from bloomscene_amd.neural_gaussians import expand_anchors
    dev = _dev()
    inp = AE.subset_inputs()
    N, K = 50, 10
    sel = inp[3].numpy().reshape(-1) > 0
    S = int(sel.sum())
    _backward(expand_anchors, inp, AE.upstreams(S, seed=99), dev)      # poison: all five upstreams, other values
    up = AE.upstreams(S, seed=7, names=names)
    got, _ = _backward(expand_anchors, inp, up, dev)
    eager, _ = _backward(OA.expand_anchors_reference, inp, up, dev)
    want = AE.restate(inp, up, K)
    _assert_exact_set(got, want, N, K, sel)
    _rule("d_gs[:, 3:6]", got[1][:, 3:], eager[1][:, 3:], want["d_gs_scale"])
    _rule("d_sr[:, 0:3]", got[5][:, :3], eager[5][:, :3], want["d_sr"][:, :3])
    _rule("d_sr[:, 3:7]", got[5][:, 3:], eager[5][:, 3:], want["d_sr"][:, 3:])
    absent = {"xyz": (got[0], got[1][:, :3], got[2]), "color": (got[4],), "opacity": (got[3],),
              "scaling": (got[1][:, 3:], got[5][:, :3]), "rot": (got[5][:, 3:],)}
    for n in NAMES:     # what only a missing upstream feeds is exactly zero
        if n not in names:
            for g in absent[n]:
                assert not g.any(), n


def test_backward_with_every_upstream_pointer_null():
    """All five NULL at once through the C ABI (autograd never calls the backward without a gradient): zeros."""
    from bloomscene_amd import _capi
    from bloomscene_amd import _operands as _ops
    from bloomscene_amd._operands import ptr
    from bloomscene_amd.neural_gaussians import expand_anchors
    dev = _dev()
    inp = AE.subset_inputs()
    N, K = 50, 10
    S = int((inp[3] > 0).sum())
    _backward(expand_anchors, inp, AE.upstreams(S, seed=99), dev)      # poison
    a, gs, go, no, co, sr = (t.to(dev).contiguous() for t in inp)
    mask = torch.empty(N * K, dtype=torch.bool, device=dev)
    scratch = _ops.scratch(_capi.lib().bsr_anchor_scratch_bytes(N, K), dev)
    import ctypes as C
    count = C.c_int(0)
    _capi.call("bsr_anchor_select", N, K, ptr(no), ptr(mask), ptr(scratch), C.byref(count), _ops.stream(dev))
    assert count.value == S
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for n in (N * 3, N * 6, N * K * 3, N * K, N * K * 3, N * K * 7)]
    _capi.call("bsr_anchor_expand_backward", N, K, S, ptr(gs), ptr(go), ptr(no), ptr(sr), ptr(scratch), None, None,
               None, None, None, *[ptr(t) for t in outs], _ops.stream(dev))
    torch.cuda.synchronize()
    for t in outs:
        assert not t.any()


# ------------------------------------------------------------------------------------------------ the fused path
def _scene(N, K, seed, keep=0.5):
    inp = list(OA.synthetic_anchor_inputs(N, K, seed=seed))
    inp[0] = inp[0] * torch.tensor([0.6, 0.35, 0.0]) + torch.tensor([0.0, 0.0, 6.0])     # in front of the camera
    if keep != 0.5:
        g = torch.Generator().manual_seed(seed + 1)
        mag = torch.rand(N * K, 1, generator=g) + 1e-3
        inp[3] = torch.where(torch.rand(N * K, 1, generator=g) < keep, mag, -mag)
    return inp


def _render(fused, inp, cam, bg, gC, reads, seed=0):
    """One forward + backward of the anchor render as one native call each way (neural_gaussians.render_anchors) or as
    the two autograd nodes of views.render_neural(fused=False), with a loss that reads the image and, directly, the
    expanded tensors named in `reads` (the result dict of render_neural carries `scaling` alone)."""
    from bloomscene_amd import GaussianRasterizer, views
    from bloomscene_amd.neural_gaussians import expand_anchors, render_anchors
    dev = _dev()
    leaves = [t.to(dev).clone().requires_grad_(True) for t in inp]
    settings = views.make_settings(cam, bg, 1)
    if fused:
        image, depth, radii, mask, xyz, rgb, opacity, scaling, rot, viewspace = render_anchors(*leaves, settings)
    else:
        rasterizer = GaussianRasterizer(raster_settings=settings)
        xyz, rgb, opacity, scaling, rot, mask = expand_anchors(*leaves)
        viewspace = torch.zeros_like(xyz, requires_grad=True)
        image, radii, depth = rasterizer(means3D=xyz, means2D=viewspace, shs=None, colors_precomp=rgb,
                                         opacities=opacity, scales=scaling, rotations=rot, cov3D_precomp=None)
    expanded = dict(zip(NAMES, (xyz, rgb, opacity, scaling, rot)))
    up = AE.upstreams(xyz.shape[0], seed=seed, names=reads)
    torch.autograd.backward([image] + [expanded[n] for n in reads], [gC] + [up[n].to(dev) for n in reads])
    return {"image": image.detach(), "depth": depth.detach(), "radii": radii, "mask": mask,
            "grads": [l.grad for l in leaves], "viewspace": viewspace.grad, "xyz": xyz}


def _assert_same_render(a, b):
    for k in ("image", "depth"):
        assert _bits(a[k], b[k]), k
    assert torch.equal(a["radii"], b["radii"]) and torch.equal(a["mask"], b["mask"])
    for name, x, y in zip(IN_NAMES, a["grads"], b["grads"]):
        assert x is not None and y is not None and _bits(x, y), name
    assert _bits(a["viewspace"], b["viewspace"])


def _camera(W, H):
    from bloomscene_amd import cameras
    from bloomscene_amd.synthetic import upstream_grads
    dev = _dev()
    cam = cameras.identity_camera(W, H, math.radians(60)).to(dev)
    return cam, torch.tensor([0.2, 0.1, 0.3], device=dev), upstream_grads(W, H, seed=3)[0].to(dev)


@pytest.mark.parametrize("reads", [(n,) for n in NAMES] + [NAMES], ids=lambda r: "+".join(r))
def test_fused_render_with_a_loss_that_reads_each_expanded_tensor(reads):
    """bsr_anchor_render_backward's `extra[]` additions (k_add_into over S * width words), one upstream at a time and all
    together: the gradients are those of the two autograd nodes, bit for bit."""
    cam, bg, gC = _camera(64, 48)
    inp = _scene(300, 10, seed=61)
    fused, two = (_render(f, inp, cam, bg, gC, reads, seed=5) for f in (True, False))
    assert int((fused["radii"] > 0).sum()) > 100
    _assert_same_render(fused, two)
    image_only = _render(True, inp, cam, bg, gC, ())
    moved = [not _bits(x, y) for x, y in zip(fused["grads"], image_only["grads"])]
    assert any(moved)       # (the direct read does reach the gradients)


def test_fused_render_when_the_size_guess_is_short_and_when_it_is_far_too_large():
    """The guess of the S-sized buffer comes from the calling thread's previous call of the same (N, K).  5 % selected,
    then 95 %: S > cap = 1.25 S0 + 1024, the buffer is asked for a second time.  Then 5 % again: the guess is the whole
    N * K, twenty times S, and the layout must follow S.  Each equals the two-node path bit for bit."""
    cam, bg, gC = _camera(64, 48)
    N, K = 600, 10
    scenes = [_scene(N, K, seed=71 + i, keep=keep) for i, keep in enumerate((0.05, 0.95, 0.05))]
    fused = [_render(True, inp, cam, bg, gC, NAMES, seed=i) for i, inp in enumerate(scenes)]   # consecutive, one thread
    S = [int(f["mask"].sum()) for f in fused]
    assert S[1] > S[0] + S[0] // 4 + 1024 and 20 * S[2] < N * K + S[2]
    # the packed buffer the outputs are views of: exactly S rows after the second request, the guessed N * K rows
    # (cap = min(1.25 S1 + 1024, N K)) when the guess was generous
    assert fused[1]["xyz"].untyped_storage().nbytes() == 15 * 4 * S[1]
    assert fused[2]["xyz"].untyped_storage().nbytes() == 15 * 4 * N * K
    for i, inp in enumerate(scenes):
        _assert_same_render(fused[i], _render(False, inp, cam, bg, gC, NAMES, seed=i))


# ------------------------------------------------------------------------------------------------ capacity mode
def _capacity_step(inp, cam, bg, gC, capacity):
    from bloomscene_amd import views
    leaves = [t.to(_dev()).clone().requires_grad_(True) for t in inp]
    res = views.render_neural(cam, *leaves, bg, capacity=capacity)
    (res["render"] * gC).sum().backward()
    return res, [l.grad for l in leaves]


def test_capacity_mode_with_every_candidate_selected():
    """BSR_FLAG_NO_READBACK with S = N * K: k_anchor_pad has no row to write.  Everything is the default mode's bits."""
    from bloomscene_amd.rasterizer import check_deferred
    cam, bg, gC = _camera(64, 48)
    N, K = 300, 10
    inp = _scene(N, K, seed=81)
    inp[3] = inp[3].abs() + 0.05
    ref, ref_g = _capacity_step(inp, cam, bg, gC, None)
    got, got_g = _capacity_step(inp, cam, bg, gC, 12 * N * K + 1024)      # (12 tiles: no frame can hold more instances)
    check_deferred()
    assert bool(got["selection_mask"].all()) and got["radii"].numel() == N * K and int((got["radii"] > 0).sum()) > 100
    for k in ("render", "depth"):
        assert _bits(got[k], ref[k]), k
    assert torch.equal(got["radii"], ref["radii"]) and torch.equal(got["selection_mask"], ref["selection_mask"])
    for name, x, y in zip(IN_NAMES, got_g, ref_g):
        assert _bits(x, y), name
    assert _bits(got["viewspace_points"].grad, ref["viewspace_points"].grad)


def test_capacity_mode_with_nothing_selected_renders_the_background():
    """BSR_FLAG_NO_READBACK with S = 0: all N * K rows are padding.  The static-shape mode has no P == 0 early return,
    so -- as include/bloomscene_anchors.h states -- the frame is the background and the depth is zero (the default mode
    returns zero images for S = 0); radii and every gradient are zero and nothing is left pending."""
    from bloomscene_amd.rasterizer import check_deferred
    cam, bg, gC = _camera(64, 48)
    N, K = 300, 10
    inp = _scene(N, K, seed=82)
    inp[3] = -inp[3].abs() - 0.05
    got, got_g = _capacity_step(inp, cam, bg, gC, 12 * N * K + 1024)
    check_deferred()
    assert not got["selection_mask"].any()
    assert got["radii"].shape == (N * K,) and not got["radii"].any()
    assert _bits(got["render"], bg.view(3, 1, 1).expand(3, 48, 64))
    assert not got["depth"].any()
    for name, g in zip(IN_NAMES, got_g):
        assert g is not None and not g.any(), name
    assert not got["viewspace_points"].grad.any()
    ref, ref_g = _capacity_step(inp, cam, bg, gC, None)      # the default mode: P == 0, zero images
    assert not ref["render"].any() and not ref["depth"].any() and ref["radii"].numel() == 0
    for g in ref_g:
        assert g is not None and not g.any()
