/*
 * bloomscene_entropy.h -- C ABI of the rate term of BloomScene's loss: the bits the context model assigns to the quantised
 * anchor attributes (`Entropy_gaussian.forward` and `Low_bound`, utils/entropy_models.py:10-50, "EM" below), and the
 * selection, masking and summing gaussian_renderer/__init__.py:100-127 ("GR") wraps around its three calls.  One kernel
 * forward, one backward; the backward recomputes everything from the operands.
 *
 * Boundary rules are those of bloomscene_densify.h: plain DEVICE pointers and ints, a hipStream_t passed as void*,
 * 0 on success, bsr_last_error() on failure, no device allocation (all scratch comes from the caller), no state kept
 * between calls.  Nothing synchronises with the host and nothing is read on the host -- x_mean is a DEVICE float -- so
 * the calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32, source order, no contraction).  Operands x, mean, scale are [n, C]; q is one value, one per row or one
 * per element; x_mean is one float; the optional weight w is [n, C / r] and applies to column j through w[i, j / r] (the
 * [m, K, 1] mask of GR:114 repeated three times: r = 3).
 *
 *   lo = x_mean - 15000 * q ;  hi = x_mean + 15000 * q          (product, then sum: EM:20-21)
 *   xc = x < lo ? lo : x ;  xc = xc > hi ? hi : xc               (torch.clamp: lo > hi gives hi, a NaN x stays NaN; EM:22)
 *   s  = scale < 1e-9 ? 1e-9 : scale                             (EM:23)
 *   upper = Phi((xc + q / 2 - mean) / s),  lower = Phi((xc - q / 2 - mean) / s),  Phi(t) = (1 + erf(t / sqrt 2)) / 2
 *   l = |upper - lower| ;  bits = -log2(l < 1e-6 ? 1e-6 : l) ;  with a weight: bits * w        (EM:24-30, GR:120)
 *
 * HOW l IS COMPUTED.  Not as written: a difference of two numbers near 1 loses everything below 2^-24.  With
 * c = xc - mean, tu = (c + q / 2) / s and tl = (c - q / 2) / s the kernel takes, for a <= b the two of tl / sqrt 2, tu / sqrt 2,
 *   0 <= a:      (erfc(a) - erfc(b)) / 2          b <= 0:   (erfc(-b) - erfc(-a)) / 2          else:   (erf(b) - erf(a)) / 2
 * and, where the bin is narrow, |q / 2s| <= 1/4 (there every difference of two cdf values cancels to q / s times their size,
 * and the gradient of q, about 1 / q, is at its largest), the integral of phi over the bin expanded at its centre m = c / s
 * with d = q / 2s:   2 d phi(m) sum_{k = 0..4} d^2k He_2k(m) / (2k + 1)!    (He_n the probabilists' Hermite polynomials; the
 * first term left out is below 3e-7 of the sum for |m| <= 6).  GUARD: for m m >= 256 the narrow bin is a zero with the sign
 * of d and the series is not formed -- exp(-m m / 2) is exactly 0 in fp32 from m m = 208 on, so no non-zero result
 * changes, while He_6 and He_8 overflow from |m| ~ 6.6e4 on and 0 * inf would be a NaN.  In particular d = 0 gives l = 0
 * for every m, an infinite one included.  So the error of l is a few units in the last place OF l for |m| < 1, on the
 * tails and for narrow bins as well; further out the fp32 roundings of c, tu, tl and m m themselves are multiplied by
 * t^2.  The largest figures of this arithmetic, measured per region on the sweep of tests/test_entropy_cpu.py (table
 * there and in docs/EXPERIMENTS.md), all at |m| in [4, 6): l 51 units of l; dx = -dmean 51, dq 45 and dscale 71 units of
 * 2^-24 of the gradient's scale; the first-order bound is 2.5 t^2 + 16 = 122 at |t| = 6.5.  Of the series the last
 * coefficient, 1 / 9!, is the least constrained by any test: its term is below 6e-7 of the sum wherever l >= 1e-6, so the
 * suite would notice it wrong by a factor of about 30 or more, no less.
 * Accuracy is judged against float64 (tests/entropy_reference.py), not against the bits of the fp32 formula above.
 *
 * OPERAND DOMAIN.  Finite operands may overflow c / s, tu or tl (mean = 1e30 over s = 1e-9): an infinite argument of Phi
 * is legal, l is then 0, 1/2 or 1 as the formula gives.  Wherever l < 1e-6 EVERY gradient is exactly 0 whatever tu and tl
 * are (no inf * 0): that covers every case in which tu and tl overflow to the same side.  With l >= 1e-6 and an infinite
 * tu or tl (a bin wider than 3.4e38 s) the gradients are unspecified.
 *
 * GRADIENT for an upstream g of bits (gl is EM:43-50: its `g < 0` pass is cancelled by its own zeroing):
 *   gl = l >= 1e-6 ? -g / (l ln 2) : 0 ;  sg = sign(upper - lower), sign(0) = 0
 *   phi(t) = exp(-t^2 / 2) / sqrt(2 pi),  du = phi(tu) / s,  dl = phi(tl) / s
 *   d/dx     =  gl sg (du - dl)            where lo <= x <= hi, else 0
 *   d/dmean  = -gl sg (du - dl)
 *   d/dscale = -gl sg (tu du - tl dl)      where scale >= 1e-9, else 0
 *   d/dq     =  gl sg (du + dl) / 2        (nothing flows through lo and hi: EM:22 detaches them); summed over the row for
 *                                          a per-row q, over everything for a single q
 *   d/dw     =  g bits                     summed over the r columns of the entry
 *   no gradient to x_mean.  With a weight, g of bits is (upstream of the product) * w.
 * du - dl is taken as -du expm1(e) (e <= 0) or dl expm1(-e) (e > 0) with e = (c / s)(q / s) = (tu^2 - tl^2) / 2, and
 * tu du - tl dl as t' (du - dl) + (q / s) d' with (t', d') the pair of the other side: no difference of two nearly equal
 * exponentials.  Below the floor (l < 1e-6) the four gradients are written as zeros without being formed.  A NaN operand
 * gives NaN bits; its gradient is unspecified.
 *
 * ROWS.  With a row mask (GR:100-101 `choose_idx`) a row whose byte is 0 is skipped before its operands are loaded: it
 * contributes nothing to the sums and its gradient rows are written as zeros.  Gradients are always dense.
 *
 * SUMS (total, count, and the gradient of a single q).  Every thread adds its terms in fp64 in index order, a workgroup
 * adds its threads in a fixed tree, each workgroup stores one fp64 partial per sum, and the workgroup that finishes last (an
 * integer ticket) adds the partials the same way and rounds once to fp32.  The grid is a function of (n, C, r) alone,
 * so the result is bit-identical from run to run.  Every term is an fp32 number, so with T = sum |term| and N terms
 *   |total - exact sum| <= 2^-24 |exact sum| + N 2^-53 T.
 * count = (rows with a non-zero mask byte, or n) * C, exact.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_ENTROPY_H_INCLUDED
#define BLOOMSCENE_ENTROPY_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* q_mode: what q points to */
#define BSR_ENTROPY_Q_SINGLE 0   /* one float */
#define BSR_ENTROPY_Q_ROW 1      /* [n] floats (BloomScene's [n, 1]) */
#define BSR_ENTROPY_Q_ELEMENT 2  /* [n, C] floats, dense */
/* g_mode of the backward: what g points to */
#define BSR_ENTROPY_G_DENSE 0    /* [n, C] floats, dense: the upstream of the bits output (bits times w) */
#define BSR_ENTROPY_G_SINGLE 1   /* one float: the upstream of total */

/* Bytes of scratch either call needs (a multiple of 256; 0 for an unsupported shape).  Opaque: the ticket and two fp64
 * partials per workgroup (the sum and, as an exact integer below 2^31, the chosen rows). */
size_t bsr_entropy_scratch_bytes(int n, int C, int r);

/* The function above for every element of every chosen row.
 *   x, mean, scale   fp32, element (i, j) at p[i * stride + j]: xs, ms, ss >= C are ROW strides in elements (a
 *                    torch.split view of a wider matrix is read in place)
 *   q                fp32, by q_mode;  x_mean one fp32 on the device
 *   rows             [n] uint8 or NULL (every row chosen)
 *   w                [n, C / r] fp32 dense, or NULL (then r must be 1)
 *   bits             [n, C] fp32 dense or NULL: bits (times w); rows not chosen are written as 0
 *   likelihood       [n, C] fp32 dense or NULL: l before its floor (for measurement); rows not chosen are written as 0
 *   total            one fp32 or NULL: the sum of bits (times w) over the chosen rows
 *   count            one int64 or NULL: chosen rows * C
 *   scratch          bsr_entropy_scratch_bytes(n, C, r) bytes, 8-byte aligned, contents ignored on entry; needed only with
 *                    total or count
 * Supported: 0 <= n < 2^31, 1 <= C, 1 <= r, C % r == 0, n * C < 2^40.  n == 0 writes total = 0 and count = 0. */
int bsr_entropy_forward(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                        const float* scale, long long ss, const float* q, int q_mode, const float* x_mean,
                        const unsigned char* rows, const float* w, float* bits, float* likelihood, float* total,
                        long long* count, void* scratch, void* stream);

/* The gradient above, recomputed from the operands (same layouts).
 *   g                fp32 by g_mode: the upstream of bits (dense) or of total (one float)
 *   dx, dmean, dscale  [n, C] fp32 dense, each fully written, each may be NULL
 *   dq               by q_mode: one float / [n] / [n, C] dense; fully written; may be NULL
 *   dw               [n, C / r] fp32 dense, fully written; may be NULL (must be NULL without w)
 *   scratch          as above; needed only for dq with BSR_ENTROPY_Q_SINGLE */
int bsr_entropy_backward(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                         const float* scale, long long ss, const float* q, int q_mode, const float* x_mean,
                         const unsigned char* rows, const float* w, const float* g, int g_mode, float* dx, float* dmean,
                         float* dscale, float* dq, float* dw, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
