/*
 * bloomscene_heads.h -- C ABI of the three anchor MLP heads of BloomScene's generate_neural_gaussians
 * (gaussian_renderer/__init__.py:151-185, "GR" below, over scene/gaussian_model.py:234-252): mlp_opacity (Tanh), mlp_cov
 * (no activation) and mlp_color (Sigmoid), each Linear(F + 4, F) -> ReLU -> Linear(F, O), evaluated on the n visible
 * anchors from feat and the view geometry, with the reshapes of GR:171/181/185 and the offset mask of GR:172 folded in,
 * forward and backward.  use_feat_bank = False (the shipped setting).
 *
 * Boundary rules are those of bloomscene_entropy.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (all memory comes from the caller), no state kept between
 * calls.  Nothing synchronises with the host and nothing is read on the host -- camera_center is a DEVICE pointer -- so
 * the calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32; every fused multiply-add below is an explicit fmaf, everything else is evaluated in source order
 * without contraction; tests/heads_reference.py evaluates the same operations in numpy).  F = feat_dim, K = n_offsets;
 * the heads h = 0, 1, 2 are opacity, cov, color with O_h = K, 7 K, 3 K outputs.
 *
 * INPUTS, per anchor row i:  feat[i * feat_stride + k], k < F (a row stride; the column stride is 1), anchor[i * 3 + c],
 * the uniform camera_center[3], and optionally offset_mask[i * K + o].
 * WEIGHTS, per head: W1 [F, F + 4], b1 [F], W2 [O_h, F], b2 [O_h], row-major exactly as nn.Linear stores them.
 *
 * GEOMETRY (GR:151-154)
 *   d = anchor - camera_center            dist = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z)        (IEEE sqrt)
 *   v = d / dist                          (three IEEE divisions)
 *   X = [feat[0 .. F), v.x, v.y, v.z, dist]                                                        (F + 4 values)
 * dist == 0 gives NaN in v and so in every output of the row, as in the reference.  There is no special case.
 *
 * LINEAR LAYERS.  Every pre-activation is the k-ascending fmaf chain started from the bias:
 *   pre1_h[j] = a after:  a = b1[j];  for k = 0 .. F + 3:  a = fmaf(X[k], W1[j][k], a)
 *   hid_h[j]  = pre1_h[j] > 0 ? pre1_h[j] : (pre1_h[j] is NaN ? pre1_h[j] : 0)          (max(pre1, 0) that keeps a NaN)
 *   pre2_h[o] = a after:  a = b2[o];  for j = 0 .. F - 1:  a = fmaf(hid_h[j], W2[o][j], a)
 * (On gfx950 the fp32-input matrix instructions compute this same chain; the kernels here use the vector unit.)
 *
 * OUTPUTS, row-major, row i at offset i * O_h -- the reshapes of GR:171/181/185:
 *   neural_opacity [n K, 1] = tanh(pre2_0) * offset_mask        (without a mask: tanh(pre2_0))
 *   scale_rot      [n K, 7] = pre2_1
 *   color          [n K, 3] = sigmoid(pre2_2)
 * ACTIVATIONS, on bsr_expf of csrc/common.h (<= 1 ulp), in forms that do not cancel near 0:
 *   tanh(x):    a = |x|
 *               a <  0.25:  u = a * a;  t = a * (1 + u * (-1/3 + u * (2/15 + u * (-17/315 + u * (62/2835)))))
 *                           (the odd series; the term left out is below 1382/155925 * 0.25^10 = 8.5e-9 of the value)
 *               a >= 0.25:  e = bsr_expf(-2 a);  t = (1 - e) / (1 + e)         (e <= 0.607: 1 - e loses under 1 bit)
 *               tanh = copysign(t, x).  Bound: 4 ulp of the result (measured against float64: tests/test_heads_cpu.py
 *               evaluates the same form); NaN gives NaN.
 *   sigmoid(x) = 1 / (1 + bsr_expf(-x))       (no difference is taken: <= 3 ulp; exp overflow gives 1 / inf = 0)
 *
 * MAPS (test and measurement only): with `maps` given the forward also writes pre1 [n, 3 F] (head-major columns) at
 * maps[0] and pre2 [n, 11 K] (columns: K of opacity, 7 K of cov, 3 K of color) at maps[n * 3 F].
 *
 * BACKWARD for upstreams g_opacity [n K, 1], g_scale_rot [n K, 7], g_color [n K, 3] (each may be NULL: that head then
 * contributes nothing).  pre1 and hid are recomputed by the chain above -- the same bits, so the gate agrees with the
 * forward's -- and so is pre2 of the opacity head; the color head uses the forward's color output s.  Per row:
 *   t = tanh(pre2_0), m = offset_mask (1 without)
 *   dpre2_0[o] = (g_opacity[o] * m[o]) * (1 - t[o] * t[o])         d offset_mask[o] = g_opacity[o] * t[o]
 *   dpre2_1[o] = g_scale_rot[o]
 *   dpre2_2[o] = (g_color[o] * s[o]) * (1 - s[o])
 *   dhid_h[j]  = a after:  a = 0;  for o = 0 .. O_h - 1:  a = fmaf(dpre2_h[o], W2[o][j], a)
 *   dpre1_h[j] = hid_h[j] > 0 ? dhid_h[j] : 0                       (the gate pre1 > 0)
 *   dX_h[k]    = a after:  a = 0;  for j = 0 .. F - 1:  a = fmaf(dpre1_h[j], W1[j][k], a)
 *   dX = (dX_0 + dX_1) + dX_2         (heads in the order opacity, cov, color; a head without upstream is left out)
 *   d feat[k] = dX[k], k < F          gv = dX[F .. F + 2], gd = dX[F + 3]
 *   s = (gv.x * v.x + gv.y * v.y) + gv.z * v.z
 *   d anchor[c] = (gv[c] - v[c] * s) / dist + gd * v[c]             (dv/dd = (I - v v^T) / dist, d dist / dd = v)
 * There is NO gradient to camera_center.
 * WEIGHT GRADIENTS are sums over the rows:
 *   dW1_h[j][k] = sum_i dpre1_h[i][j] * X[i][k]        db1_h[j] = sum_i dpre1_h[i][j]
 *   dW2_h[o][j] = sum_i dpre2_h[i][o] * hid_h[i][j]    db2_h[o] = sum_i dpre2_h[i][o]
 * in a FIXED order that depends on (n, F, K) alone: the rows are cut into ranges of BSR_HEADS_CHUNK rows; one thread per
 * element adds its range in ascending row order in fp64 (a = fma((double)dpre, (double)x, a) from 0 -- the product of two
 * fp32 values is exact there; the biases a = a + (double)dpre) and stores one partial per range, rounded to fp32; a last
 * pass adds the partials of an element in fp64 in ascending range order, starting from the first, and rounds once.
 * No float atomics: bit-identical from run to run.  A head without upstream is not evaluated: its weight gradients are
 * exactly zero and d offset_mask is zero when it is the opacity head.
 *
 * DEVIATIONS FROM THE REFERENCE.  (1) The summation order of every product is the one stated above, not the GEMM
 * library's.  (2) tanh and sigmoid are the forms above, not libm's.  (3) The weight gradients are deterministic.
 *
 * SUPPORTED: 1 <= F <= 64, 1 <= K <= 16, n >= 0, n * max(7 K, F + 4) < 2^31.  Anything else is an error that names the
 * argument.  n == 0 launches nothing and writes zeros to the weight gradients asked for.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_HEADS_H_INCLUDED
#define BLOOMSCENE_HEADS_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_HEADS_MAX_F 64
#define BSR_HEADS_MAX_K 16
#define BSR_HEADS_CHUNK 256 /* rows per range of the weight-gradient sums */
#define BSR_HEADS_OPACITY 0
#define BSR_HEADS_COV 1
#define BSR_HEADS_COLOR 2

/* The twelve weight tensors, head[BSR_HEADS_OPACITY | _COV | _COLOR]; device pointers, read in place. */
typedef struct bsr_heads_weights {
	struct {
		const float* w1; /* [F, F + 4] */
		const float* b1; /* [F] */
		const float* w2; /* [O_h, F] */
		const float* b2; /* [O_h] */
	} head[3];
} bsr_heads_weights;

/* Their gradients, dense with the same shapes, fully written; any pointer may be NULL (that gradient is not stored). */
typedef struct bsr_heads_weight_grads {
	struct {
		float* w1;
		float* b1;
		float* w2;
		float* b2;
	} head[3];
} bsr_heads_weight_grads;

/* Bytes of scratch the backward needs when a weight gradient is asked for (a multiple of 256; 0 for arguments out of
 * range).  Opaque: the per-row X, hid, dpre1, dpre2 the row pass leaves for the sums, then one partial per range and
 * element. */
size_t bsr_anchor_heads_scratch_bytes(int n, int F, int K);

/* The function above.
 *   feat, feat_stride   fp32 rows of F values, feat_stride (>= F) elements apart
 *   anchor              [n, 3] dense;  camera_center  3 floats on the device;  offset_mask  [n, K] dense or NULL
 *   w                   the weights (a HOST struct of device pointers)
 *   neural_opacity, color, scale_rot   [n K], [n K, 3], [n K, 7] dense, fully written
 *   maps                n * (3 F + 11 K) floats (see MAPS) or NULL */
int bsr_anchor_heads_forward(int n, int F, int K, const float* feat, long long feat_stride, const float* anchor,
                             const float* camera_center, const float* offset_mask, const bsr_heads_weights* w,
                             float* neural_opacity, float* color, float* scale_rot, float* maps, void* stream);

/* The gradients above.
 *   color               the forward's color output
 *   g_opacity, g_color, g_scale_rot    the upstreams, dense, each may be NULL
 *   d_feat [n, F], d_anchor [n, 3], d_offset_mask [n, K]   dense, fully written; each may be NULL (d_offset_mask
 *                       needs offset_mask)
 *   dw                  NULL, or the weight gradients wanted.  With every one of them NULL the row pass alone runs and
 *                       the scratch is not touched (it may be NULL)
 *   scratch             bsr_anchor_heads_scratch_bytes(n, F, K) bytes, 16-byte aligned, contents ignored on entry */
int bsr_anchor_heads_backward(int n, int F, int K, const float* feat, long long feat_stride, const float* anchor,
                              const float* camera_center, const float* offset_mask, const bsr_heads_weights* w,
                              const float* color, const float* g_opacity, const float* g_color, const float* g_scale_rot,
                              float* d_feat, float* d_anchor, float* d_offset_mask, const bsr_heads_weight_grads* dw,
                              void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
