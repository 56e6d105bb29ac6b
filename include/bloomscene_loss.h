/*
 * bloomscene_loss.h -- C ABI of the photometric term of BloomScene's loss (bloomscene.py:284-287 over utils/loss.py:83-134,
 * "UL" below): the mean absolute difference of two images and the mean of their SSIM map under an 11 x 11 Gaussian window,
 *
 *   loss = (1 - lambda) * L1(img, gt) + lambda * (1 - ssim(img, gt)),
 *
 * with its gradient to the first image.  One kernel forward, one backward; the forward leaves three per-pixel partial
 * derivatives for the backward, which convolves them once more.
 *
 * Boundary rules are those of bloomscene_entropy.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (all memory comes from the caller), no state kept between
 * calls.  Nothing synchronises with the host and nothing is read on the host -- the upstream gradient is a DEVICE float -- so
 * the calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32, source order, no contraction; every parenthesis below is an association the kernels and the
 * restatement of tests/photometric_reference.py keep).  img and gt are dense [B, C, H, W]; N = B * C * H * W.
 *
 * WINDOW.  w[0..10] is the fp32 vector UL:91-93 gives for gaussian(11, 1.5): BSR_PHOTOMETRIC_W0 .. _W5 below, then
 * mirrored (w[k] = w[10 - k]).  conv(t) is the separable, zero-padded convolution of one [H, W] plane, rows first:
 *
 *   h[y][x] = acc after:  acc = 0;  for k = 0 .. 10:  acc = acc + w[k] * t[y][x + k - 5]      (t = 0 outside 0 <= x + k - 5 < W)
 *   conv(t)[y][x] = acc after:  acc = 0;  for k = 0 .. 10:  acc = acc + w[k] * h[y + k - 5][x]   (h = 0 outside 0 <= y + k - 5 < H)
 *
 * A tap outside the image contributes w[k] * 0, it is not skipped.
 * DEVIATION FROM THE REFERENCE.  UL:96-99 convolves with the 2-D window fl(w[i] * w[j]) and leaves the order of the 121
 * terms to the convolution library.  The separable form is a different rounding of the same sum, not a bit-for-bit copy:
 * the claim (tests/test_photometric_cpu.py) is that it is no further from the float64 value of UL's formula than UL's own
 * fp32 evaluation is.
 *
 * THE SSIM MAP (UL:114-129).
 *   mu1 = conv(img)   mu2 = conv(gt)   e11 = conv(img * img)   e22 = conv(gt * gt)   e12 = conv(img * gt)
 *   p12 = mu1 * mu2   q1 = mu1 * mu1   q2 = mu2 * mu2
 *   s1 = e11 - q1     s2 = e22 - q2    s12 = e12 - p12
 *   a = 2 * p12 + C1          b = 2 * s12 + C2          c = (q1 + q2) + C1          d = (s1 + s2) + C2
 *   C1 = (float)1e-4, C2 = (float)9e-4
 *   ab = a * b        cd = c * d       m = ab / cd                                    (IEEE division)
 * The cancellation in s1, s2, s12 belongs to the formula and is kept.
 *
 * THE THREE PARTIALS the forward saves, dm/dmu1, dm/de11, dm/de12 with mu2, e22 held (plane order in `partials`):
 *   pMu  = ((2 * mu2) * (b - a)) / cd  -  (((2 * mu1) * ab) * (d - c)) / (cd * cd)
 *   pE11 = -(ab / (cd * d))
 *   pE12 = (2 * a) / cd
 *
 * SCALARS.  L1 = sum |img - gt| / N (the difference and its absolute value in fp32), S = sum m / N.  Both sums: every
 * thread adds its terms in fp64 in a fixed order, a workgroup adds its threads in a fixed tree, each workgroup stores one
 * fp64 partial per sum, and the workgroup that draws the last integer ticket adds the partials the same way.  Then, in fp64,
 *   L1 = sum1 / N,  S = sum2 / N,  loss = (1 - lambda) * L1 + lambda * (1 - S),   out[3] = {loss, L1, S} each rounded to fp32 once.
 * The grid is a function of the shape alone: bit-identical from run to run.
 *
 * GRADIENT to img for an upstream g of loss (one DEVICE float).  With the two fp32 factors
 *   kl = (1 - lambda) / (float)N          ks = -lambda / (float)N
 *   sg = sign(img - gt), sign(0) = 0
 *   inner = (conv(pMu) + (2 * img) * conv(pE11)) + gt * conv(pE12)
 *   grad  = g * (kl * sg + ks * inner)
 * (the window is symmetric and the padding zero, so the transposed convolution is conv itself).  There is NO gradient to
 * gt.  The gradient of S alone is this call with lambda = 1 and -g.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_LOSS_H_INCLUDED
#define BLOOMSCENE_LOSS_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* w[0] .. w[5] of gaussian(11, 1.5) in fp32; w[10 - k] = w[k] */
#define BSR_PHOTOMETRIC_W0 0x1.0d956cp-10f
#define BSR_PHOTOMETRIC_W1 0x1.f1fe02p-8f
#define BSR_PHOTOMETRIC_W2 0x1.26eb18p-5f
#define BSR_PHOTOMETRIC_W3 0x1.bff0fep-4f
#define BSR_PHOTOMETRIC_W4 0x1.b43c3ep-3f
#define BSR_PHOTOMETRIC_W5 0x1.10656p-2f
#define BSR_PHOTOMETRIC_C1 1e-4f
#define BSR_PHOTOMETRIC_C2 9e-4f
/* plane order of `partials` */
#define BSR_PHOTOMETRIC_P_MU 0
#define BSR_PHOTOMETRIC_P_E11 1
#define BSR_PHOTOMETRIC_P_E12 2

/* Bytes of scratch the forward needs (a multiple of 256; 0 for an unsupported shape).  Opaque: the ticket and two fp64
 * partials per workgroup. */
size_t bsr_photometric_scratch_bytes(int B, int C, int H, int W);

/* The function above.
 *   img, gt     [B, C, H, W] fp32 dense
 *   partials    [3, B, C, H, W] fp32 dense, fully written, or NULL: nothing is saved (no backward will follow)
 *   ssim_map    [B, C, H, W] fp32 dense, fully written with m, or NULL (for measurement)
 *   out         three fp32: loss, L1, S
 *   scratch     bsr_photometric_scratch_bytes(B, C, H, W) bytes, 8-byte aligned, contents ignored on entry
 * Supported: B, C >= 0, H, W >= 1, N < 2^31.  B * C == 0 writes out = {0, 0, 0} and nothing else. */
int bsr_photometric_forward(int B, int C, int H, int W, const float* img, const float* gt, float lambda, float* partials,
                            float* ssim_map, float* out, void* scratch, void* stream);

/* The gradient above from the partials of a forward on the same img, gt.
 *   g           one fp32 on the device: the upstream of loss
 *   grad        [B, C, H, W] fp32 dense, fully written */
int bsr_photometric_backward(int B, int C, int H, int W, const float* img, const float* gt, const float* partials,
                             float lambda, const float* g, float* grad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
