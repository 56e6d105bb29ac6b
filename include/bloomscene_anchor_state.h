/*
 * bloomscene_anchor_state.h -- C ABI of the two per-anchor blocks of a BloomScene training iteration that are driven by
 * the visible-anchor index list:
 *   the PROLOGUE of generate_neural_gaussians, gaussian_renderer/__init__.py:34-46 ("GR"): the six x[visible_mask]
 *   gathers over the model properties get_anchor (scene/gaussian_model.py:394-399, "GM"; Quantize_anchor,
 *   utils/encodings.py:215-227, "ENC"), get_scaling (GM:342-346), get_mask (GM:348-353), get_mask_anchor (GM:355-364)
 *   and mask_anchor_rate (GR:46) -- evaluated on the n visible rows only, forward and backward;
 *   the EPILOGUE GaussianModel.training_statis (GM:742-759): the densification statistics, in place.
 *
 * Boundary rules are those of bloomscene_heads.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (all memory comes from the caller), no state kept between
 * calls.  Nothing synchronises with the host and nothing is read on the host -- the bounds are DEVICE pointers -- so the
 * calls can be captured into a hipGraph.  No float atomics anywhere: every result is bit-identical from run to run.
 * Purely additive: BSR_VERSION stays 4.
 *
 * THE INDEX LIST.  idx is int64 [n], as bsr_visible_filter_indices writes it: STRICTLY ASCENDING, every value in [0, N).
 * That is a precondition of the results, not of memory safety: a value outside [0, N) is never dereferenced -- its
 * output row is zero, its mask_anchor is false, and it contributes to no gradient and no accumulator -- and a list that
 * is not ascending makes bsr_anchor_visible_backward miss rows (they stay zero) and lets two writers meet on a row of
 * bsr_anchor_accumulate, always inside the tensors.
 *
 * ---- A. THE PROLOGUE (fp32, evaluated in source order without contraction; tests/anchor_state_reference.py restates it)
 * N anchors, F = feat_dim, K = n_offsets.  For output row i with r = idx[i]:
 *
 *   anchor[i][c]  (GM:394-399 / ENC:215-227, then GR:34)
 *       interval_c = ((max_c - min_c) * fl32(1 / 65535)) + fl32(1e-6)
 *       a = _anchor[r][c] - min_c, b = interval_c, q = torch.div(a, b, rounding_mode='floor'), which is
 *           b == 0:  q = a / b
 *           else     mod = fmodf(a, b) (exact);  div = (a - mod) / b;  if (mod != 0 && (b < 0) != (mod < 0)) div = div - 1
 *                    div != 0:  q = floorf(div);  if (div - q > 0.5f) q = q + 1
 *                    div == 0:  q = copysignf(0, a / b)
 *       (NOT floorf(a / b): the quotient of an exact multiple can round below the integer)
 *       q = q < 0 ? 0 : (q > 65535 ? 65535 : q)       (a NaN stays NaN)
 *       anchor = q * interval_c + min_c                 (two roundings)
 *   feat[i][k] = _anchor_feat[r * feat_stride + k],  grid_offsets[i][k][c] = _offset[r][k][c]      (GR:36-37; copies)
 *   grid_scaling[i][c] = bsr_expf(_scaling[r][c]), c < 6      (GM:346, GR:38; the pinned exp of csrc/common.h, <= 1 ulp)
 *   binary_grid_masks[i][k] = s > 0.01f ? 1.0f : 0.0f,  s = 1 / (1 + bsr_expf(-_mask[r][k]))        (GM:352-353, GR:43;
 *       the sigmoid form of bloomscene_heads.h, <= 3 ulp; a NaN gives 0)
 *   mask_anchor[i] = any k with binary_grid_masks[i][k] == 1  (one byte, 0 / 1)                     (GM:361-363, GR:44-45)
 *   mask_anchor_rate = fl32(count) / fl32(n), count = the number of true mask_anchor, an INTEGER sum (GR:46); n == 0: NaN
 *
 * DEVIATIONS FROM THE REFERENCE.  (1) The reference's forward value of the mask is fl(fl(b - s) + s) for b = 0 / 1, which
 * can be 1 +- 2^-24; ours is exactly b.  (2) The decision s > 0.01 is taken on the sigmoid form above; torch's sigmoid can
 * decide the other way within a few ulp of x = logit(0.01) = -4.59512.  (3) grid_scaling uses bsr_expf, not the device
 * library's exp: both are <= 1 ulp.
 *
 * BACKWARD for upstreams g_anchor [n, 3], g_feat [n, F], g_offsets [n, K, 3], g_scaling [n, 6], g_masks [n, K] (dense;
 * each may be NULL: that gradient is then zero everywhere).  The gradients are DENSE over the N rows and fully written:
 *   row r = idx[i]:   d_anchor[r] = g_anchor[i]           (straight-through, ENC:226-227; nothing goes to the bounds)
 *                     d_feat[r] = g_feat[i]               d_offset[r] = g_offsets[i]
 *                     d_scaling[r][c] = g_scaling[i][c] * grid_scaling[i][c]       (the forward's value, as exp backward)
 *                     d_mask[r][k] = (g_masks[i][k] * s) * (1 - s)                 (s recomputed: the same bits)
 *   every other row:  0
 * One thread writes each element, so there is nothing to add up.  mask_anchor and the rate have no gradient.
 *
 * ---- B. THE EPILOGUE (GM:743-759), in place, no gradient
 * For visible i with r = idx[i] in [0, N):
 *   opacity_accum[r] += a after:  a = 0;  for k = 0 .. K - 1:  o = neural_opacity[i K + k];  a = a + (o < 0 ? 0 : o)
 *                       (a NaN stays a NaN, as t[t < 0] = 0 leaves it)                                    (GM:743-747)
 *   anchor_demon[r] += 1                                                                                  (GM:748)
 * For every candidate c = i K + k with selection[c] != 0, with j = the number of selected candidates before c (its rank in
 * candidate order: it indexes the rasterizer's M gaussians), if j < M and filter[j] (radii[j] > 0, or the bool itself):
 *   offset_gradient_accum[r K + k] += sqrtf(gx * gx + gy * gy), (gx, gy) = grad[j][0 .. 1]               (GM:750-758)
 *                                     (three roundings and a correctly rounded root)
 *   offset_denom[r K + k] += 1                                                                            (GM:759)
 * j >= M is skipped and never read: the padded static-shape form of the renderer (padding rows have radius 0) and an
 * undersized M need no second path.  The ranks are an integer prefix count in a fixed order: a count per scan block of
 * BSR_ANCHOR_STATE_SCAN candidates, then every block adds the counts before it.  Two kernels.  Every target has one
 * writer (idx is ascending), so the updates are plain read-modify-writes.
 *
 * SUPPORTED: 1 <= F <= 64, 1 <= K <= 16, 0 <= n <= N, N * max(F, 3 K) < 2^31, M >= 0.  Anything else is an error that
 * names the argument.  n == 0 launches nothing, except that bsr_anchor_visible_forward writes the NaN rate and
 * bsr_anchor_visible_backward the zeros.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_ANCHOR_STATE_H_INCLUDED
#define BLOOMSCENE_ANCHOR_STATE_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_ANCHOR_STATE_MAX_F 64
#define BSR_ANCHOR_STATE_MAX_K 16
#define BSR_ANCHOR_STATE_SCAN 1024 /* candidates per scan block of bsr_anchor_accumulate */

/* A, forward (GR:34-46).
 *   idx                        [n] int64 (see THE INDEX LIST)
 *   anchor [N, 3], bound_min [3], bound_max [3], offset [N, K, 3], scaling [N, 6], mask [N, K]    dense
 *   feat, feat_stride          rows of F values, feat_stride (>= F) elements apart
 *   out_anchor [n, 3], out_feat [n, F], out_offsets [n, K, 3], out_scaling [n, 6], out_masks [n, K]    dense, fully written
 *   out_mask_anchor            [n] bytes, 4-byte aligned;  out_rate  one float */
int bsr_anchor_visible_forward(int N, int n, int F, int K, const long long* idx, const float* anchor, const float* bound_min,
                               const float* bound_max, const float* feat, long long feat_stride, const float* offset,
                               const float* scaling, const float* mask, float* out_anchor, float* out_feat,
                               float* out_offsets, float* out_scaling, float* out_masks, unsigned char* out_mask_anchor,
                               float* out_rate, void* stream);

/* A, backward (what autograd runs for GR:34-46: the exp and sigmoid backward over all N rows, ENC:226-227, six zero-filled
 * dense gradients and an index_add_ each).
 *   mask                       the forward's input [N, K] (read only where d_mask is asked for)
 *   grid_scaling               the forward's out_scaling [n, 6] (read only where d_scaling is asked for)
 *   g_*                        the upstreams, dense, each may be NULL
 *   d_anchor [N, 3], d_feat [N, F], d_offset [N, K, 3], d_scaling [N, 6], d_mask [N, K]    dense, fully written; each may
 *                              be NULL (that gradient is not computed) */
int bsr_anchor_visible_backward(int N, int n, int F, int K, const long long* idx, const float* mask,
                                const float* grid_scaling, const float* g_anchor, const float* g_feat,
                                const float* g_offsets, const float* g_scaling, const float* g_masks, float* d_anchor,
                                float* d_feat, float* d_offset, float* d_scaling, float* d_mask, void* stream);

/* Bytes of scratch bsr_anchor_accumulate needs: one count per scan block (a multiple of 256; 0 for n <= 0 and for
 * arguments out of range). */
size_t bsr_anchor_accumulate_scratch_bytes(int n, int K);

/* B (GM:743-759).
 *   neural_opacity [n K], selection [n K] bytes (0 / not 0), grad [M, 3]    dense
 *   filter, filter_is_bool     [M] int32 radii (the filter is radii > 0), or with filter_is_bool != 0 [M] bytes
 *   opacity_accum [N], anchor_demon [N], offset_gradient_accum [N K], offset_denom [N K]    updated in place
 *   scratch                    bsr_anchor_accumulate_scratch_bytes(n, K) bytes, 4-byte aligned, contents ignored on entry */
int bsr_anchor_accumulate(int N, int n, int K, int M, const long long* idx, const float* neural_opacity,
                          const unsigned char* selection, const void* filter, int filter_is_bool, const float* grad,
                          float* opacity_accum, float* anchor_demon, float* offset_gradient_accum, float* offset_denom,
                          void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
