/*
 * bloomscene_depth_loss.h -- C ABI of the depth-prior regularisation of BloomScene's loss (bloomscene.py:295-325 over
 * utils/loss.py:26-80,170-202, "UL" below): the two min/max normalisations, HuberL1 with edge-aware weights from the
 * ground-truth image, CMD as it is called (a batch of one) and bilateral_filter(spatial_sigma = 2, color_sigma = 5),
 *
 *   loss = wv * Lv + wd * Ld + ws * Ls,
 *
 * with its gradient to the rendered depth.  At most three kernels forward (extrema -> M -> sums) and two backward; the
 * forward leaves a small stats block (the extrema, M, S, the tie counts, the sums) so that the backward repeats no
 * reduction of the forward's.
 *
 * Boundary rules are those of bloomscene_loss.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (all memory comes from the caller), no state kept between
 * calls.  Nothing synchronises with the host and nothing is read on the host -- the upstream gradient is a DEVICE float -- so
 * the calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32, source order, no contraction; every parenthesis below is an association the kernels and the numpy
 * evaluation of tests/depth_prior_reference.py keep).  D (rendered) and P (prior) are dense [H, W]; rgb is read in place
 * as rgb[y * sy + x * sx + c * sc], c = 0..2 (three element strides: a transposed view costs no copy).  HW = H * W.
 *
 * NORMALISATION (bloomscene.py:299-305), when `normalise` is set:
 *   rgD = (maxD - minD) + 1e-8f      r = (D - minD) / rgD          (IEEE division)
 *   rgP = (maxP - minP) + 1e-8f      o = (P - minP) / rgP
 * otherwise r = D, o = P.
 *
 * VALUE TERM (UL:170-202, HuberL1 with tresh = 0.2, "scalar"; needs H, W >= 2):
 *   e = r - o      l1 = |e|      M = max l1      d = 0.2f * M
 *   h = l1 where l1 >= d, otherwise (e * e + d * d) / (2 * d)       (a select: with M = 0 the 0 / 0 is never chosen)
 *   gx[y][x] = ((|c0 - c0'| + |c1 - c1'|) + |c2 - c2'|) / 3 over rgb[y][x] and rgb[y][x + 1], for x < W - 1
 *   gy[y][x] the same over rgb[y][x] and rgb[y + 1][x], for y < H - 1
 *   ex = exp(-gx) (0 for x = W - 1)      ey = exp(-gy) (0 for y = H - 1)
 *   Sx = sum of ex * h over x < W - 1    Sy = sum of ey * h over y < H - 1
 *   nx = H * (W - 1)      ny = (H - 1) * W      Lv = Sx / nx + Sy / ny                       (fp64)
 * UL's reshape(512, 512) is the call's own H, W.
 *
 * DISTRIBUTION TERM (UL:26-60 for a batch of one: every central moment is (0 + 1e-6f)^k on both sides):
 *   clamp(x) = x < -1e6f ? -1e6f : (x > 1e6f ? 1e6f : x)            (NaN passes through)
 *   ec = clamp(r) - clamp(o)      t = |ec| + 1e-6f      pw = t * t      pw = pw > 1e6f ? 1e6f : pw
 *   S = sum pw      K = 4 * sqrt(HW * (1e-6f)^2 + 1e-6)      Ld = sqrt(min(S, 1e6) + 1e-6) + K     (fp64)
 *
 * SMOOTHNESS TERM (UL:63-80 with spatial_sigma = 2, color_sigma = 5, a 5 x 5 window, replicate padding):
 *   n(p, i, j) = (clamp(py + i - 2, 0, H - 1), clamp(px + j - 2, 0, W - 1))
 *   delta = r[p] - r[n(p, i, j)]      tap = (sk[i][j] * exp(-(|delta| / 50))) * (delta * delta)
 *   b[p] = acc after: acc = 0; for i = 0 .. 4: for j = 0 .. 4: acc = acc + tap            (the bilateral map)
 *   Ls = (sum b) / HW                                                                      (fp64)
 * sk is the normalised fp32 kernel of UL:65-68; its six distinct values, by (i - 2)^2 + (j - 2)^2, are BSR_DEPTH_PRIOR_SK*.
 *
 * SUMS AND OUTPUT.  Sx, Sy, S, sum b (and Q below): every thread adds its terms in fp64 in a fixed order, a workgroup adds
 * its threads in a fixed tree, each workgroup stores one fp64 partial per sum, and the workgroup that draws the last
 * integer ticket adds the partials the same way.  The extrema, M and their tie counts are exact whatever the order.
 *   out[4] = {(wv * Lv + wd * Ld) + ws * Ls, Lv, Ld, Ls}, formed in fp64, each rounded to fp32 once.
 * A term that is off is not evaluated and is 0 in both places.  The grids are functions of the shape alone: bit-identical
 * from run to run.
 *
 * GRADIENT to D for an upstream g of out[0] (one DEVICE float).  sign(0) = 0.  Per pixel, G = dloss / dr:
 *   a  = ex / (float)nx + ey / (float)ny
 *   Gv = a * sign(e)                      where l1 >= d
 *        a * (e / d)                      otherwise
 *        + sign(e) * qM                   where l1 == M;   qM = (float)((double)0.2f * Q / cntM),
 *          Q = sum over the pixels with l1 < d of (double)(a * (0.5f - (e * e) / (2 * (d * d)))),  cntM = #{l1 == M}
 *   Gd = sign(ec) * (t / sd)              where |r| <= 1e6f and t * t <= 1e6f and S <= 1e6, otherwise 0 (torch's clamp rule)
 *        sd = (float)sqrt(min(S, 1e6) + 1e-6)
 *   t'(x) = exp(-(|x| / 50)) * (2 * x - sign(x) * ((x * x) / 50))
 *   A1 = acc after: for i, for j:  acc = acc + sk[i][j] * t'(r[q] - r[n(q, i, j)])
 *   A2 = acc after: for every pixel p of the image with |py - qy|, |px - qx| <= 2, rows first: for every (i, j), i first,
 *        with n(p, i, j) = q:  acc = acc + sk[i][j] * t'(r[p] - r[q])
 *        (one tap per p in the interior, where A2 = -A1; several within two pixels of the border, where replicate padding
 *        maps several taps of p onto q: a gather per destination pixel)
 *   Gs = (A1 - A2) / (float)HW
 *   G  = (wv * Gv + wd * Gd) + ws * Gs            (a term that is off is left out)
 * Without `normalise`, grad = g * G.  With it, sG = sum (double)G and sGr = sum (double)G * (double)r (fixed-order fp64 as
 * above), and
 *   qmin = (float)((sGr - sG) / rgD / cntMin)      qmax = (float)(-sGr / rgD / cntMax)
 *   grad = g * ((G / rgD + (D == minD ? qmin : 0)) + (D == maxD ? qmax : 0))
 * -- the even sharing among ties of torch's full-reduction min() / max() backward.  Ties are the normal case: every pixel
 * the rasterizer left empty has depth exactly 0.  There is NO gradient to P or rgb.
 *
 * DEVIATIONS FROM THE REFERENCE.  (1) No NaN / inf asserts (UL:34-37 are four host waits): a NaN input gives NaN scalars.
 * (2) exp is bsr_expf of csrc/common.h (<= 1 ulp), not libm's.  (3) The mean over three channels and the 25-tap sum have
 * the association written above, not torch's; the pixel sums are fp64.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_DEPTH_LOSS_H_INCLUDED
#define BLOOMSCENE_DEPTH_LOSS_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sk by (i - 2)^2 + (j - 2)^2 = 0, 1, 2, 4, 5, 8 */
#define BSR_DEPTH_PRIOR_SK0 0x1.02d50cp-4f
#define BSR_DEPTH_PRIOR_SK1 0x1.c8d656p-5f
#define BSR_DEPTH_PRIOR_SK2 0x1.93285p-5f
#define BSR_DEPTH_PRIOR_SK4 0x1.39fab6p-5f
#define BSR_DEPTH_PRIOR_SK5 0x1.1515f8p-5f
#define BSR_DEPTH_PRIOR_SK8 0x1.7ce05p-6f
#define BSR_DEPTH_PRIOR_TRESH 0.2f
#define BSR_DEPTH_PRIOR_COLOR_DIV 50.0f /* 2 * color_sigma^2 */
/* bits of `terms` */
#define BSR_DEPTH_PRIOR_VALUE 1
#define BSR_DEPTH_PRIOR_DOMIN 2
#define BSR_DEPTH_PRIOR_SMOOTH 4
/* plane order of `maps` */
#define BSR_DEPTH_PRIOR_MAP_R 0
#define BSR_DEPTH_PRIOR_MAP_H 1
#define BSR_DEPTH_PRIOR_MAP_B 2
/* bytes of the stats block the forward leaves for the backward (opaque, 8-byte aligned) */
#define BSR_DEPTH_PRIOR_STATS_BYTES 128

/* Bytes of scratch either call needs (a multiple of 256; 0 for an unsupported shape).  Opaque: tickets and fp64
 * partials per workgroup. */
size_t bsr_depth_prior_scratch_bytes(int H, int W);

/* The function above.
 *   D, P              [H, W] fp32 dense
 *   rgb, sy, sx, sc   fp32 and its three element strides; NULL allowed when the value term is off
 *   terms             which terms are on (BSR_DEPTH_PRIOR_VALUE | _DOMIN | _SMOOTH); wv, wd, ws their weights
 *   maps              [3, H, W] fp32 dense, fully written with r, h, b (h and b zero when their term is off), or NULL
 *   out               four fp32: loss, Lv, Ld, Ls
 *   stats             BSR_DEPTH_PRIOR_STATS_BYTES bytes, 8-byte aligned, for the backward
 *   scratch           bsr_depth_prior_scratch_bytes(H, W) bytes, 16-byte aligned, contents ignored on entry
 * Supported: H, W >= 1 (>= 2 with the value term on), H * W < 2^31. */
int bsr_depth_prior_forward(int H, int W, const float* D, const float* P, const float* rgb, long long sy, long long sx,
                            long long sc, int terms, float wv, float wd, float ws, int normalise, float* maps, float* out,
                            void* stats, void* scratch, void* stream);

/* The gradient above from the stats of a forward with the same arguments.
 *   g           one fp32 on the device: the upstream of out[0]
 *   grad        [H, W] fp32 dense, fully written
 *   scratch     as for the forward (its own: the forward's contents are not needed) */
int bsr_depth_prior_backward(int H, int W, const float* D, const float* P, const float* rgb, long long sy, long long sx,
                             long long sc, int terms, float wv, float wd, float ws, int normalise, const void* stats,
                             const float* g, float* grad, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
