"""The photometric loss on the GPU (include/bloomscene_loss.h, bloomscene_amd/loss.py) against the fp32 restatement of
tests/photometric_reference.py: the SSIM map and the gradient bit for bit, the three scalars within one fp32 unit of the
exact sums of the restatement's elements.  No conv2d runs on the GPU here (tools/bench_photometric.py times the eager
lines).

Shapes (B, C, H, W), relative to the kernels' tile of 32 x 16 pixels: one pixel; every tap but a few in the padding; one
full window; exactly one tile; one pixel over the tile in both directions; a ragged multi-tile shape with B > 1 whose
halos cross tile edges both ways; narrow and tall (three tile rows, one ragged); [3, 512, 512] once, 1536 workgroups
for the ticket; and 8193 small planes of two tiles once, two tiles more than there are workgroups, so that the first two
workgroups walk on to a second tile with a halo to stage (the grid-stride path).  Inputs: the scene kinds of the
restatement, "hdr" with values in [-2, 6] among them.  Every (shape, scene) is evaluated once and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import photometric_reference as PR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TW, TH = 32, 16      # BSR_LOSS_TW, BSR_LOSS_TH of csrc/loss.hip
LAMBDA = 0.2
SMALL = ((1, 1, 1, 1), (1, 3, 3, 4), (1, 3, 11, 11), (1, 3, TH, TW), (1, 3, TH + 1, TW + 1), (2, 3, 37, 53),
         (1, 3, 2 * TH + 3, 5))
BIG = (1, 3, 512, 512)
MAX_BLOCKS = 16384   # BSR_LOSS_MAX_BLOCKS: more tiles than this and a workgroup walks several
STRIDE = (2731, 3, 17, 5)   # 8193 planes of two tiles, the lower one ragged with the upper one's rows in its halo: 16386 tiles
CASES = [(s, k) for s in SMALL for k in PR.SCENES] + [(BIG, "noise"), (STRIDE, "noise")]


def _L():
    import bloomscene_amd.loss as L
    return L


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(img_d, gt_d, lam, upstream):
    """photometric_loss forward + backward on fresh leaves -> (out[3] as numpy float32, grad as numpy)."""
    L = _L()
    leaf = img_d.clone().requires_grad_(True)
    loss, (l1, s) = L.photometric_loss(leaf, gt_d, lam, return_terms=True)
    (loss if upstream == 1.0 else upstream * loss).backward()
    return np.array([loss.item(), l1.item(), s.item()], dtype=np.float32), leaf.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """Inputs, the fp32 restatement and the kernels' results for one (shape, scene), computed once and left unchanged."""
    L = _L()
    img, gt = PR.scene(kind, *shape, seed=1)
    c = SimpleNamespace(shape=shape, kind=kind, img=img, gt=gt, ref=PR.evaluate(img.numpy(), gt.numpy(), LAMBDA, np.float32))
    c.img_d, c.gt_d = img.to(DEV), gt.to(DEV)
    c.map = L.ssim_map(c.img_d, c.gt_d).cpu().numpy()
    c.out, c.grad = _run(c.img_d, c.gt_d, LAMBDA, 1.0)
    c.out_again, c.grad_again = _run(c.img_d, c.gt_d, LAMBDA, 1.0)
    _, c.grad_scaled = _run(c.img_d, c.gt_d, LAMBDA, 3.5)
    return c


def _ids(case):
    return "x".join(map(str, case[0])) + "-" + case[1]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_map_and_gradient_are_the_restatement_bit_for_bit(case):
    c = _case(*case)
    assert c.map.shape == c.shape and c.grad.shape == c.shape
    assert np.isfinite(c.ref.map).all() and np.isfinite(c.ref.grad).all()
    assert (_bits(c.map) == _bits(c.ref.map)).all(), float(np.abs(c.map - c.ref.map).max())
    assert (_bits(c.grad) == _bits(c.ref.grad)).all(), float(np.abs(c.grad - c.ref.grad).max())
    # a non-unit upstream: (3.5 * loss).backward()
    assert (_bits(c.grad_scaled) == _bits(np.float32(3.5) * c.ref.grad_unit)).all()
    if c.ref.grad.size > 1:
        assert np.abs(c.ref.grad).max() > 0


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_scalars_within_one_unit_of_the_exact_sums_and_repeatable(case):
    c = _case(*case)
    for name, got, exact in zip(("loss", "L1", "S"), c.out, c.ref.out):
        unit = float(np.spacing(np.float32(abs(exact)))) if exact != 0 else 2.0 ** -149
        print(f"{name}: kernel {float(got)!r} exact {exact!r} distance in units {abs(float(got) - exact) / unit:.3f}")
        assert abs(float(got) - exact) <= unit, (name, float(got), exact)
    assert (_bits(c.out) == _bits(c.out_again)).all()
    assert (_bits(c.grad) == _bits(c.grad_again)).all()


def test_the_grid_stride_shape_has_more_tiles_than_workgroups():
    B, C, H, W = STRIDE
    per_plane = -(-H // TH) * -(-W // TW)
    assert per_plane > 1 and H % TH and B * C * per_plane > MAX_BLOCKS
    c = _case(STRIDE, "noise")
    wrapped = c.grad.reshape(B * C, H, W)[(MAX_BLOCKS // per_plane):]      # the planes whose tiles are second tiles
    assert wrapped.shape[0] >= 1 and np.abs(wrapped).min() > 0
    lib = __import__("bloomscene_amd._capi", fromlist=["lib"]).lib()
    assert lib.bsr_photometric_scratch_bytes(B, C, H, W) == lib.bsr_photometric_scratch_bytes(1, 1, MAX_BLOCKS * TH, TW)


@pytest.mark.parametrize("case", [((2, 3, 37, 53), "smooth"), ((1, 3, TH + 1, TW + 1), "flat")], ids=_ids)
def test_ssim_and_the_two_ends_of_lambda(case):
    L = _L()
    c = _case(*case)
    leaf = c.img_d.clone().requires_grad_(True)
    s = L.ssim(leaf, c.gt_d)
    assert s.dim() == 0 and s.requires_grad
    assert _bits(s.item()) == _bits(c.out[2])                        # return_terms' S
    s.backward()
    out1, grad1 = _run(c.img_d, c.gt_d, 1.0, 1.0)
    assert (_bits(leaf.grad.cpu().numpy()) == _bits(-grad1)).all()   # loss = 1 - S at lambda = 1
    ref1 = PR.evaluate(c.img.numpy(), c.gt.numpy(), 1.0, np.float32)
    assert (_bits(grad1) == _bits(ref1.grad)).all()
    assert abs(float(out1[0]) - (1.0 - c.ref.out[2])) <= float(np.spacing(np.float32(1.0 - c.ref.out[2])))
    assert _bits(out1[1]) == _bits(c.out[1]) and _bits(out1[2]) == _bits(c.out[2])   # the terms do not depend on lambda
    out0, grad0 = _run(c.img_d, c.gt_d, 0.0, 1.0)
    assert _bits(out0[0]) == _bits(out0[1]) == _bits(c.out[1])        # loss = L1 at lambda = 0
    ref0 = PR.evaluate(c.img.numpy(), c.gt.numpy(), 0.0, np.float32)
    assert (_bits(grad0) == _bits(ref0.grad)).all()
    # [C, H, W] is [1, C, H, W]
    if c.shape[0] == 1:
        out3, grad3 = _run(c.img_d[0], c.gt_d[0], LAMBDA, 1.0)
        assert (_bits(out3) == _bits(c.out)).all() and (_bits(grad3) == _bits(c.grad[0])).all()


def test_through_autograd():
    L = _L()
    c = _case((2, 3, 37, 53), "smooth")
    N = c.img.numel()
    # the image comes out of an upstream op (x / 2 and 2 * g are exact)
    x = (c.img_d * 2).requires_grad_(True)
    loss = L.photometric_loss(x * 0.5, c.gt_d, LAMBDA)
    assert loss.dim() == 0 and loss.requires_grad and _bits(loss.item()) == _bits(c.out[0])
    loss.backward()
    assert (_bits(x.grad.cpu().numpy()) == _bits(np.float32(0.5) * c.ref.grad)).all()
    # one autograd node, and the terms are detached
    loss, (l1, s) = L.photometric_loss(c.img_d.clone().requires_grad_(True), c.gt_d, LAMBDA, return_terms=True)
    assert type(loss.grad_fn).__name__ == "_PhotometricBackward" and not l1.requires_grad and not s.requires_grad
    # a non-contiguous image and target
    img_nc = c.img_d.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    gt_nc = c.gt_d.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not img_nc.is_contiguous() and not gt_nc.is_contiguous()
    leaf = img_nc.detach().requires_grad_(True)
    loss = L.photometric_loss(leaf, gt_nc, LAMBDA)
    loss.backward()
    assert _bits(loss.item()) == _bits(c.out[0]) and (_bits(leaf.grad.cpu().numpy()) == _bits(c.grad)).all()
    # the second image's gradient is refused, not zero
    with pytest.raises(NotImplementedError):
        L.photometric_loss(c.img_d, c.gt_d.clone().requires_grad_(True))
    # no gradient wanted: no partials are allocated (they would be 3 N floats)
    leaf = c.img_d.clone().requires_grad_(True)
    torch.cuda.synchronize()
    for wanted in (False, True):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if wanted:
            loss = L.photometric_loss(leaf, c.gt_d, LAMBDA)
        else:
            with torch.no_grad():
                loss = L.photometric_loss(leaf, c.gt_d, LAMBDA)
            assert not loss.requires_grad and _bits(loss.item()) == _bits(c.out[0])
            plain = L.photometric_loss(c.img_d, c.gt_d, LAMBDA)       # nothing requires grad
            assert not plain.requires_grad
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        assert (peak >= 3 * N * 4) == wanted, (wanted, peak, N)


def test_forward_and_backward_replay_from_a_graph_without_a_host_wait():
    """Forward and backward captured with torch.cuda.graph after one warm-up call (capture raises on any host wait) and
    replayed on new pixel values: bit-equal to the direct call."""
    L = _L()
    shape = (2, 3, 37, 53)
    c, c2 = _case(shape, "smooth"), _case(shape, "noise")
    img = c.img_d.clone().requires_grad_(True)
    gt = c.gt_d.clone()

    def step():
        loss, (l1, s) = L.photometric_loss(img, gt, LAMBDA, return_terms=True)
        grad, = torch.autograd.grad(3.5 * loss, [img])
        return loss, l1, s, grad

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
        img.copy_(c2.img_d)
        gt.copy_(c2.gt_d)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.detach().clone() for t in captured]
    direct = step()
    torch.cuda.synchronize()
    for a, b in zip(replayed, direct):
        assert torch.equal(a, b.detach())
    assert (_bits(replayed[3].cpu().numpy()) == _bits(c2.grad_scaled)).all()
    assert _bits(replayed[0].item()) == _bits(c2.out[0])


def test_library_owns_no_device_memory():
    """Every device byte of a forward + backward comes from the caller, here torch's allocator: memory in use outside
    torch's pool does not grow across a call whose partials are 75 MB, and torch's own accounting shows them."""
    L = _L()
    _case((1, 1, 1, 1), "noise")                         # library and streams: set up
    B, C, H, W = shape = (1, 3, 1080, 1920)
    N = B * C * H * W
    gen = torch.Generator(device=DEV).manual_seed(3)
    img = torch.rand(shape, device=DEV, generator=gen).requires_grad_(True)
    gt = torch.rand(shape, device=DEV, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    free0, total = torch.cuda.mem_get_info()
    outside0 = total - free0 - torch.cuda.memory_reserved()
    alloc0 = torch.cuda.memory_allocated()
    loss = L.photometric_loss(img, gt, LAMBDA)
    loss.backward()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    outside1 = total - free1 - torch.cuda.memory_reserved()
    # (growth only: the HIP runtime may release memory of its own meanwhile)
    assert outside1 - outside0 < (8 << 20), (outside0, outside1)
    assert torch.cuda.max_memory_allocated() - alloc0 >= 3 * N * 4          # the partials are on torch's books
    assert torch.isfinite(loss).item() and torch.isfinite(img.grad).all().item()
    lib = __import__("bloomscene_amd._capi", fromlist=["lib"]).lib()
    assert lib.bsr_photometric_scratch_bytes(B, C, H, W) == 256 + 3 * 60 * 68 * 16
    assert lib.bsr_photometric_scratch_bytes(1, 3, 0, 5) == 0


def test_empty_and_refused_shapes():
    L = _L()
    empty = torch.zeros(0, 3, 4, 5, device=DEV, requires_grad=True)
    loss, (l1, s) = L.photometric_loss(empty, torch.zeros(0, 3, 4, 5, device=DEV), LAMBDA, return_terms=True)
    assert loss.item() == 0.0 and l1.item() == 0.0 and s.item() == 0.0
    loss.backward()
    assert empty.grad.shape == (0, 3, 4, 5)
    from bloomscene_amd import _capi
    one = torch.zeros(4, device=DEV)
    assert _capi.lib().bsr_photometric_forward(1, 1, 0, 1, one.data_ptr(), one.data_ptr(), 0.2, None, None, one.data_ptr(),
                                               None, None) == 1
    assert "H, W >= 1" in _capi.last_error()
