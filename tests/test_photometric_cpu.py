"""The restatement the GPU tests of the photometric loss compare with (tests/photometric_reference.py), checked on the CPU:
the window constants against the reference's construction, the float64 restatement against the conv2d formula of
utils/loss.py:114-132 with torch autograd, the fp32 restatement's distance from float64 against fp32 eager conv2d's, the
argument rejections of bloomscene_amd.loss, and that importing it needs no GPU.

The measured figures are in the two tests' docstrings and in docs/EXPERIMENTS.md."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import photometric_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((7, 5), (37, 53), (128, 128))     # (H, W), C = 3
LAMBDA = 0.2


def _window_1d():
    """utils/loss.py:91-93 for (11, 1.5): python floats into a float32 tensor, divided by its float32 sum."""
    gauss = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    return gauss / gauss.sum()


def _window_2d(channels, dtype):
    """utils/loss.py:96-99, the outer product of the float32 1-D window with itself, one copy per channel, formed in
    ``dtype``.  In float64 every product of two float32 numbers is exact; in float32 (the reference as it runs) each is
    rounded, a relative 2^-24 a tap -- the deviation include/bloomscene_loss.h states."""
    w = _window_1d().to(dtype).unsqueeze(1)
    return w.mm(w.t()).unsqueeze(0).unsqueeze(0).expand(channels, 1, 11, 11).contiguous()


def _eager(img, gt, lam, dtype, window_dtype):
    """bloomscene.py:285-286 over utils/loss.py:83-84 and :114-132 in eager torch of ``dtype`` on the CPU, with the 2-D
    window formed in ``window_dtype`` and cast to ``dtype``.  -> map, loss, grad (numpy)."""
    img = img.to(dtype).clone().requires_grad_(True)
    gt = gt.to(dtype)
    ch = img.shape[1]
    win = _window_2d(ch, window_dtype).to(dtype)
    mu1 = F.conv2d(img, win, padding=5, groups=ch)
    mu2 = F.conv2d(gt, win, padding=5, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img * img, win, padding=5, groups=ch) - mu1_sq
    sigma2_sq = F.conv2d(gt * gt, win, padding=5, groups=ch) - mu2_sq
    sigma12 = F.conv2d(img * gt, win, padding=5, groups=ch) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    loss = (1.0 - lam) * torch.abs(img - gt).mean() + lam * (1.0 - ssim_map.mean())
    grad, = torch.autograd.grad(loss, img)
    return ssim_map.detach().numpy(), float(loss.detach()), grad.numpy()


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    img, gt = PR.scene(kind, 1, 3, H, W, seed=1)
    map64, loss64, grad64 = _eager(img, gt, LAMBDA, torch.float64, torch.float64)
    map32, _, grad32 = _eager(img, gt, LAMBDA, torch.float32, torch.float32)     # the reference as it runs
    return dict(img=img, gt=gt, map64=map64, loss64=loss64, grad64=grad64, map32=map32, grad32=grad32,
                rounded_window=_eager(img, gt, LAMBDA, torch.float64, torch.float32),
                r64=PR.evaluate(img.numpy(), gt.numpy(), LAMBDA, np.float64),
                r32=PR.evaluate(img.numpy(), gt.numpy(), LAMBDA, np.float32))


def test_window_constants_are_the_reference_construction_bit_for_bit():
    ours = PR.window(np.float32)
    theirs = _window_1d().numpy()
    assert theirs.dtype == np.float32 and ours.dtype == np.float32
    assert (ours.view(np.uint32) == theirs.view(np.uint32)).all(), (ours, theirs)
    assert (ours == ours[::-1]).all()
    hdr = open(os.path.join(ROOT, "include", "bloomscene_loss.h")).read()
    for k, h in enumerate(PR.WINDOW_HEX):
        assert f"#define BSR_PHOTOMETRIC_W{k} {h}f\n" in hdr     # the header carries the same six literals


def _errors(r, truth):
    """(map, loss, grad / max|grad|) distances of an evaluation from a (map, loss, grad) float64 truth."""
    m, loss, grad = truth
    return (float(np.abs(r.map.astype(np.float64) - m).max()), abs(r.out[0] - loss),
            float(np.abs(r.grad.astype(np.float64) - grad).max()) / float(np.abs(grad).max()))


@pytest.mark.parametrize("kind", PR.SCENES)
def test_float64_restatement_is_the_conv2d_formula(kind):
    """Bar 1e-10 absolute: the fp32 form's worst map error is 2e-3, 3.3e4 fp32 units; the same amplification of float64
    rounding is 4e-12, and a wrong term is at least 1e-6.

    WHICH 2-D WINDOW.  The bar is met, and asserted, against conv2d with the reference's window construction (the outer
    product of its float32 1-D window) carried out in float64, where every product is exact: measured at most 3.6e-12
    (map), 2.9e-14 (loss), 1.1e-12 (gradient) over the nine cases.  Against the window as the reference itself holds it
    -- the products rounded to float32, then cast -- NO separable form can meet it: the two windows differ by a relative
    2^-24 in every tap, which is the deviation the header states, and the distance is then up to 3.3e-6 (map), 8.5e-8
    (loss), 8.7e-6 (gradient): the tap rounding through the cancellation of s1, s2, s12, not a term of the formula.  That distance is printed, and bounded by what the tap rounding can do."""
    for H, W in SHAPES:
        c = _case(kind, H, W)
        r = c["r64"]
        assert r.map.dtype == np.float64 and r.grad.dtype == np.float64 and float(np.abs(c["grad64"]).max()) > 0
        e_map, e_loss, e_grad = _errors(r, (c["map64"], c["loss64"], c["grad64"]))
        print(f"float64 agreement {kind} {H}x{W}: map {e_map:.3g} loss {e_loss:.3g} grad/max|grad| {e_grad:.3g}")
        assert e_map <= 1e-10 and e_loss <= 1e-10 and e_grad <= 1e-10
        # The rounded window: each of the five moments moves by at most 2^-24 of a sum of non-negative terms <= 1 (the
        # inputs are in [0, 1.01]), and the map amplifies a moment's error by at most 1 / C2 + 2 / C1 < 3.3e4 / 1.5.
        # (hdr: second moments up to 36, but variances of order 1 in place of C2: measured below 1e-6, far inside.)
        w_map, w_loss, w_grad = _errors(r, c["rounded_window"])
        print(f"  ... against the float32-rounded 2-D window: map {w_map:.3g} loss {w_loss:.3g} grad/max|grad| {w_grad:.3g}")
        assert w_map <= 5 * 2.0 ** -24 * 3.3e4 and w_loss <= w_map + 1e-10


@pytest.mark.parametrize("kind", PR.SCENES)
def test_fp32_restatement_is_no_further_from_float64_than_eager_conv2d(kind):
    """Pooled over the three shapes (a single tiny shape can fall either way): the largest elementwise error of the map and
    the largest gradient error over max|grad64|, no margin; the eager side is the reference as it runs (float32 window,
    float32 conv2d on the CPU).  Holds against the float64 formula with either 2-D window (see above); both are asserted.
    Measured on the CPU:

        scene    map, restatement   map, eager   gradient, restatement   gradient, eager
        noise    2.5e-6             6.5e-6       3.8e-7                  1.1e-6
        smooth   2.6e-4             8.0e-4       5.6e-5                  1.5e-4
        flat     5.1e-4             2.0e-3       2.6e-4                  4.9e-4
        hdr      2.6e-7             6.7e-7       1.3e-7                  2.9e-7
    """
    for which in ("exact window products", "float32-rounded window products"):
        ours_map = ours_grad = eager_map = eager_grad = 0.0
        for H, W in SHAPES:
            c = _case(kind, H, W)
            assert c["r32"].map.dtype == np.float32 and c["r32"].grad.dtype == np.float32
            m64, _, g64 = (c["map64"], c["loss64"], c["grad64"]) if which.startswith("exact") else c["rounded_window"]
            scale = float(np.abs(g64).max())
            ours_map = max(ours_map, float(np.abs(c["r32"].map.astype(np.float64) - m64).max()))
            eager_map = max(eager_map, float(np.abs(c["map32"].astype(np.float64) - m64).max()))
            ours_grad = max(ours_grad, float(np.abs(c["r32"].grad.astype(np.float64) - g64).max()) / scale)
            eager_grad = max(eager_grad, float(np.abs(c["grad32"].astype(np.float64) - g64).max()) / scale)
        print(f"fp32 against float64 ({which}), {kind}: map restatement {ours_map:.3g} eager {eager_map:.3g}; "
              f"gradient restatement {ours_grad:.3g} eager {eager_grad:.3g}")
        assert ours_map <= eager_map
        assert ours_grad <= eager_grad


def test_restatement_scalars_and_upstream():
    """out is built from exact sums; the gradient is linear in the upstream g; lambda = 0 and 1 reduce to the terms."""
    img, gt = (t.numpy() for t in PR.scene("smooth", 2, 3, 9, 13))
    r = PR.evaluate(img, gt, LAMBDA, np.float64)
    lam = float(np.float64(LAMBDA))
    assert r.out[1] == math.fsum(np.abs(img.astype(np.float64) - gt).ravel().tolist()) / img.size
    assert r.out[0] == (1.0 - lam) * r.out[1] + lam * (1.0 - r.out[2])
    r3 = PR.evaluate(img, gt, LAMBDA, np.float64, g=3.5)
    assert np.allclose(r3.grad, 3.5 * r.grad, rtol=1e-14, atol=0)
    r0, r1 = PR.evaluate(img, gt, 0.0, np.float64), PR.evaluate(img, gt, 1.0, np.float64)
    assert r0.out[0] == r0.out[1] and r1.out[0] == 1.0 - r1.out[2]
    assert np.allclose(np.abs(r0.grad) * img.size, (img != gt).astype(np.float64), rtol=1e-15, atol=0)


def test_argument_rejections_on_cpu_tensors():
    from bloomscene_amd.loss import photometric_loss, ssim
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    for fn in (photometric_loss, ssim):
        with pytest.raises(TypeError):
            fn(a.double(), b)                       # a dtype comes before the device
        with pytest.raises(TypeError):
            fn(a, b.half())
        with pytest.raises(TypeError):
            fn(a.numpy(), b)
        with pytest.raises(NotImplementedError):
            fn(a, b.clone().requires_grad_(True))   # no silent zero for the second image
        with pytest.raises(ValueError, match="one shape"):
            fn(a, torch.rand(3, 8, 9))
        with pytest.raises(ValueError):
            fn(a[0], b[0])                          # [H, W]
        with pytest.raises(ValueError, match="no CPU path"):
            fn(a, b)
        with pytest.raises(ValueError, match="no CPU path"):
            fn(a.unsqueeze(0), b.unsqueeze(0))
    with pytest.raises(NotImplementedError):
        ssim(a, b, window_size=7)
    with pytest.raises(NotImplementedError):
        ssim(a, b, size_average=False)
    with pytest.raises(TypeError):
        ssim(a.double(), b, window_size=7)          # still the dtype first


def test_import_needs_no_gpu():
    code = ("import os; os.environ['HIP_VISIBLE_DEVICES'] = ''; os.environ['CUDA_VISIBLE_DEVICES'] = ''\n"
            "import bloomscene_amd.loss as L, bloomscene_amd._capi as c\n"
            "assert c._lib is None and callable(L.photometric_loss) and callable(L.ssim)\n"
            "import torch; assert not torch.cuda.is_initialized()\n")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
