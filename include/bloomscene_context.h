/*
 * bloomscene_context.h -- C ABI of the context model's head of BloomScene's generate_neural_gaussians
 * (gaussian_renderer/__init__.py, "GR" below): the grid MLP mlp_grid (scene/gaussian_model.py:254-258,
 * Linear(D, H) -> ReLU -> Linear(H, O)) on the hash-grid encoding of the n visible anchors (GR:76, GR:135), the three
 * adaptive step sizes (GR:82-84, GR:137-139), the noise injection of training (GR:87-97) and the STE_multistep quantiser
 * of rendering (GR:140-142 over utils/encodings.py:196-212), forward and backward.
 *
 * Boundary rules are those of bloomscene_heads.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (all memory comes from the caller), no state kept between
 * calls.  Nothing synchronises with the host and nothing is read on the host -- the three means are DEVICE pointers --
 * so the calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32; every fused multiply-add below is an explicit fmaf, everything else is evaluated in source order
 * without contraction; tests/context_reference.py evaluates the same operations in numpy).
 *   D = width of the encoding (encoding_xyz.output_dim), H = hidden width (2 F in the reference, its own argument here),
 *   F = feat_dim, K = n_offsets, O = 2 F + 12 + 6 K + 3.
 *
 * INPUTS, per anchor row i:  enc[i * enc_stride + k], k < D (a row stride; the column stride is 1).
 * WEIGHTS: W1 [H, D], b1 [H], W2 [O, H], b2 [O], row-major exactly as nn.Linear stores them, read live.
 *
 * LINEAR LAYERS -- the chains of bloomscene_heads.h:
 *   pre1[j] = a after:  a = b1[j];  for k = 0 .. D - 1:  a = fmaf(enc[k], W1[j][k], a)
 *   hid[j]  = pre1[j] > 0 ? pre1[j] : (pre1[j] is NaN ? pre1[j] : 0)                  (max(pre1, 0) that keeps a NaN)
 *   pre2[o] = a after:  a = b2[o];  for j = 0 .. H - 1:  a = fmaf(hid[j], W2[o][j], a)
 *   context [n, O] = pre2 verbatim, row i at offset i * O.  Its column blocks are those of the split of GR:77-78:
 *     mean F | scale F | mean_scaling 6 | scale_scaling 6 | mean_offsets 3 K | scale_offsets 3 K | the three adjustments
 *
 * STEP SIZES (GR:82-84), c = 0, 1, 2 for feat, scaling, offsets, adj[c] = pre2[O - 3 + c]:
 *   Q[c] = q_c * (1 + tanh(adj[c]))                   q = (0.25, 2.5e-4, 5e-2) in the reference, three floats here
 *   tanh is the form of bloomscene_heads.h (<= 4 ulp, on bsr_expf).  Output Q [n, 3].
 *
 * TRAINING TAIL (GR:87-97), per attribute and only where its x and noise are given -- x_0 = feat [n, F],
 * x_1 = grid_scaling [n, 6], x_2 = grid_offsets [n, 3 K], each read through a row stride; noise_c dense like x_c:
 *   out_c[k] = x_c[k] + noise_c[k] * (Q[c] + 1e-6f)              (the sum in brackets, the product, the sum: no fmaf)
 * The noise is the CALLER's randn_like: no random number is drawn here, a call is a pure function of its arguments.
 *
 * INFERENCE TAIL (GR:140-142: STE_multistep with use_clamp = True, tau = 1), per attribute where its x is given; the
 * means m_c are three device scalars (pc._anchor_feat.mean() ...).  For every element, in this order:
 *   lo = m_c - 15000 * Q[c]          hi = m_c + 15000 * Q[c]
 *   x  = x < lo ? lo : x;  x = x > hi ? hi : x                    (min(max(x, lo), hi); a NaN x stays NaN)
 *   r  = rintf(x / Q[c])                                          (IEEE division, ties to even)
 *   Qq = r * Q[c]
 *   out_c[k] = Qq + tanh(x - Qq) * Q[c]
 * This form evaluates layer 1 in full and only the LAST THREE ROWS of W2 (the same chains: the same Q bits as the
 * training form); it writes no context and has no gradient (the reference detaches it).
 *
 * MAPS (test and measurement only): with `maps` given the training form also writes pre1 [n, H].
 *
 * BACKWARD of the training form, for upstreams g_context [n, O], g_Q [n, 3] and g_out_c like out_c (each may be NULL
 * and then costs nothing).  pre1, hid and adj are recomputed by the chains above -- the same bits, so the gate agrees
 * with the forward's.  Per row:
 *   dQ[c]    = a after:  a = g_Q[c] (0 without);  for k ascending:  a = fmaf(g_out_c[k], noise_c[k], a)
 *   t        = tanh(adj[c])
 *   dadj[c]  = (dQ[c] * q_c) * (1 - t * t)
 *   dpre2[o] = g_context[o] (0 without), and dpre2[O - 3 + c] = g_context[O - 3 + c] + dadj[c]
 *              (with neither g_Q nor any g_out_c given, adj and dadj are not evaluated: dpre2 = g_context)
 *   dhid[j]  = a after:  a = 0;  for o = 0 .. O - 1:  a = fmaf(dpre2[o], W2[o][j], a)
 *   dpre1[j] = hid[j] > 0 ? dhid[j] : 0                          (the gate pre1 > 0)
 *   d enc[k] = a after:  a = 0;  for j = 0 .. H - 1:  a = fmaf(dpre1[j], W1[j][k], a)
 * The gradient to x_c is g_out_c itself: nothing is written for it.  Noise, q and the means get no gradient.
 * WEIGHT GRADIENTS are sums over the rows:
 *   dW1[j][k] = sum_i dpre1[i][j] * enc[i][k]      db1[j] = sum_i dpre1[i][j]
 *   dW2[o][j] = sum_i dpre2[i][o] * hid[i][j]      db2[o] = sum_i dpre2[i][o]
 * in the FIXED order of bloomscene_heads.h, which depends on (n, D, H, F, K) alone: ranges of BSR_CONTEXT_CHUNK rows; one
 * thread per element adds its range in ascending row order in fp64 (a = fma((double)dpre, (double)x, a) from 0; the
 * biases a = a + (double)dpre) and stores one partial per range, rounded to fp32; a last pass adds the partials of an
 * element in fp64 in ascending range order, starting from the first, and rounds once.  No float atomics: bit-identical
 * from run to run.
 *
 * DEVIATIONS FROM THE REFERENCE.  (1) The summation order of every product is the one stated above, not the GEMM
 * library's.  (2) tanh is the form above, not libm's.  (3) The weight gradients are deterministic.  (4) The random
 * numbers stay with the caller.
 *
 * SUPPORTED: 1 <= D, H <= 128, 1 <= F <= 64, 1 <= K <= 16, n >= 0, n * max(O, D) < 2^31.  Anything else is an error that
 * names the argument.  n == 0 launches nothing and writes zeros to the weight gradients asked for.  A launch whose
 * workgroup needs more LDS than the device gives one is refused with an error.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_CONTEXT_H_INCLUDED
#define BLOOMSCENE_CONTEXT_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_CONTEXT_MAX_D 128
#define BSR_CONTEXT_MAX_H 128
#define BSR_CONTEXT_MAX_F 64
#define BSR_CONTEXT_MAX_K 16
#define BSR_CONTEXT_CHUNK 256 /* rows per range of the weight-gradient sums */

/* The four weight tensors; device pointers, read in place. */
typedef struct bsr_context_weights {
	const float* w1; /* [H, D] */
	const float* b1; /* [H] */
	const float* w2; /* [O, H] */
	const float* b2; /* [O] */
} bsr_context_weights;

/* Their gradients, dense with the same shapes, fully written; any pointer may be NULL (that gradient is not stored). */
typedef struct bsr_context_weight_grads {
	float* w1;
	float* b1;
	float* w2;
	float* b2;
} bsr_context_weight_grads;

/* Bytes of scratch the backward needs when a weight gradient is asked for (a multiple of 256; 0 for arguments out of
 * range).  Opaque: the per-row enc, hid, dpre1, dpre2 the row pass leaves for the sums, then one partial per range and
 * element. */
size_t bsr_context_scratch_bytes(int n, int D, int H, int F, int K);

/* The training form.
 *   enc, enc_stride     fp32 rows of D values, enc_stride (>= D) elements apart
 *   w                   the weights (a HOST struct of device pointers)
 *   q_feat, q_scaling, q_offsets   the three base step sizes
 *   feat, scaling, offsets         x_c with their row strides (>= F, 6, 3 K), each NULL or given together with
 *   noise_feat, noise_scaling, noise_offsets   its noise, dense [n, F], [n, 6], [n, 3 K], and with
 *   out_feat, out_scaling, out_offsets         its output, dense like the noise, fully written
 *   context [n, O], Q [n, 3]       dense, fully written
 *   maps                n * H floats (see MAPS) or NULL */
int bsr_context_head_forward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                             const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                             const float* feat, long long feat_stride, const float* scaling, long long scaling_stride,
                             const float* offsets, long long offsets_stride, const float* noise_feat,
                             const float* noise_scaling, const float* noise_offsets, float* context, float* Q,
                             float* out_feat, float* out_scaling, float* out_offsets, float* maps, void* stream);

/* The gradients above.
 *   noise_*             the forward's noise; needed where the matching g_out_* is given
 *   g_context, g_Q, g_out_feat, g_out_scaling, g_out_offsets   the upstreams, dense, each may be NULL
 *   d_enc [n, D]        dense, fully written; may be NULL
 *   dw                  NULL, or the weight gradients wanted.  With every one of them NULL the row pass alone runs and
 *                       the scratch is not touched (it may be NULL)
 *   scratch             bsr_context_scratch_bytes(n, D, H, F, K) bytes, 16-byte aligned, contents ignored on entry */
int bsr_context_head_backward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                              const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                              const float* noise_feat, const float* noise_scaling, const float* noise_offsets,
                              const float* g_context, const float* g_Q, const float* g_out_feat,
                              const float* g_out_scaling, const float* g_out_offsets, float* d_enc,
                              const bsr_context_weight_grads* dw, void* scratch, void* stream);

/* The inference form.
 *   feat, scaling, offsets         x_c with their row strides, each NULL or given together with its output
 *   feat_mean, scaling_mean, offsets_mean   one float each on the device (needed where the matching x_c is given)
 *   Q                   [n, 3] dense, fully written, or NULL */
int bsr_context_quantise_forward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                                 const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                                 const float* feat, long long feat_stride, const float* scaling, long long scaling_stride,
                                 const float* offsets, long long offsets_stride, const float* feat_mean,
                                 const float* scaling_mean, const float* offsets_mean, float* Q, float* out_feat,
                                 float* out_scaling, float* out_offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
