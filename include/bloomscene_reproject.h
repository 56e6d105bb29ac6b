/*
 * bloomscene_reproject.h -- C ABI of the point-cloud reprojection of the scene-lifting stage: the two geometric steps of
 * BloomScene.generate_pcd (bloomscene.py:428-656, "BS") for gfx950.
 *
 *   bsr_warp_points    a coloured point cloud -> image, depth, mask, mask_hf and each point's pixel in one camera
 *                      (BS:479-504 per generation pose, BS:621-648 per training frame)
 *   bsr_lift_pixels    a depth frame + an image -> world points and colours of the selected pixels
 *                      (BS:470-472, BS:545-551)
 *
 * bsr_warp_points IS NOT scipy.interpolate.griddata, which the reference calls (a Delaunay triangulation of every
 * projected point).  It is the pure function written out below: a bilinear splat behind a soft z-buffer, resolved per
 * pixel, with a small inverse-square-distance fill.  It has a visibility test the reference lacks (use_z_test = 0 turns
 * it off: then every point contributes, as in the reference).  The tolerance the Python wrapper defaults to, 0.05, is a
 * CHOICE, not a tuned value.  The hit mask, the two mask filters, mask_hf, the validity rule and the rounded coordinates
 * are the reference's, exactly.
 *
 * Boundary rules are those of the sibling headers: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (scratch is the caller's), no state kept between calls,
 * nothing read on the host: the calls only enqueue (capturable into a graph).  The camera (K, R, T, or the two inverses)
 * is a HOST array of doubles, copied into the kernel-argument block.  No float atomics: every accumulation is an integer
 * atomic, exact in any order, so every output is bit-identical from run to run.  The unit is built with
 * -ffp-contract=off: no expression below is fused.  Purely additive: BSR_VERSION stays 4.
 *
 * ---- bsr_warp_points: the function ----
 * Point i is x = (double)points[i * point_stride + k * comp_stride], k = 0, 1, 2; its colour colors[3 i + k] (fp32).
 * camera[21] = K (row-major 3 x 3), R (row-major 3 x 3), T (3), world-to-camera: x_cam = R x + T.
 *
 * 1. PROJECTION, in fp64.  x_cam[j] = ((R[j][0] x[0] + R[j][1] x[1]) + R[j][2] x[2]) + T[j];
 *    p[j] = (K[j][0] x_cam[0] + K[j][1] x_cam[1]) + K[j][2] x_cam[2];  u = p[0] / p[2], v = p[1] / p[2], z = p[2].
 *    The point is VALID iff z > 0, 0 <= u <= W - 1, 0 <= v <= H - 1 (BS:482-486; a NaN fails a comparison) and its three
 *    colours are finite.  pixel[i] = rint(v) * W + rint(u), rounding half to even as np.round does (BS:488); -1 for an
 *    invalid point.  zf = (float)z is the point's depth from here on.
 * 2. HIT MASK.  hit[pixel[i]] = 1 for every valid point (BS:494-495).
 * 3. SOFT Z-BUFFER.  x0 = floor(u), y0 = floor(v), fx = u - x0, fy = v - y0.  The point's FOOTPRINT is the pixels
 *    (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) with the fp64 weights (1 - fx)(1 - fy), fx (1 - fy),
 *    (1 - fx) fy, fx fy, those of them with weight > 0 that lie in the frame.  zmin[q] = the minimum of zf over every
 *    valid point whose footprint has q: an integer atomic minimum of the bit pattern, which orders as the value does
 *    because zf >= 0.  The point CONTRIBUTES to q iff (double)zf <= (double)zmin[q] * (1.0 + z_tolerance), or
 *    always when use_z_test is 0.
 * 4. SPLAT.  A contributing (point, q) pair adds rint(clamp(w * x * 2^S, -2^62, 2^62)) -- fp64, w * x first, half to even
 *    -- to five signed 64-bit sums of q, x = 1, r, g, b, (double)zf, with an integer atomic add.  S =
 *    BSR_REPROJECT_SHIFT = 28.  OVERFLOW: w <= 1, so a contribution is at most 2^(S + 12) = 2^40 in magnitude while
 *    |x| <= 2^12, and 2^22 such points on one pixel stay within 2^62 < 2^63.  Beyond that domain the sums wrap (two's
 *    complement): still a pure function, no longer a mean.  The clamp only keeps the conversion defined for a huge x.
 *    A pixel whose weight sum is > 0 is RESOLVED: value = (float)((double)sum_x / (double)sum_1) for r, g, b and depth.
 * 5. FILL.  known = the maximum of hit over the 9 x 9 window clipped to the frame (BS:496).  A pixel that is known and
 *    not resolved takes, per channel and for depth, (float)(sum_k g_k value_k / sum_k g_k) over the RESOLVED pixels k of
 *    its clipped 9 x 9 window with (double)depth_k <= (1.0 + z_tolerance) * (double)dmin, dmin the smallest resolved depth
 *    of the window (all resolved pixels when use_z_test is 0); g_k = 1.0 / (double)(dy^2 + dx^2); both sums in fp64,
 *    row-major over the window, g_k * value_k rounded before it is added.  Only values of step 4 are read, never filled
 *    ones.  THE WINDOW HOLDS A RESOLVED PIXEL: it holds a hit pixel h; h is the footprint pixel nearest to the point that
 *    hit it, with weight >= 1/4; so some point has h in its footprint, the nearest of them passes its own z-test at h,
 *    and h is resolved unless that point's own weight there rounds to 0 at scale 2^S (below 2^-29: then another pixel
 *    holds almost all of it).  Where the window holds none after all, the value is 0: there is no division by zero.
 *    A pixel that is neither resolved nor known has the value 0.
 * 6. BORDER RING (BS:493, BS:638-641, which repair griddata's hull; kept so that results stay comparable).  Pixel (r, c)
 *    shows the value of steps 4-5 at (clamp(r, 1, H - 2), clamp(c, 1, W - 2)): the identity except in the outermost row
 *    and column, which is all the reference's ring of width 2 changes.  Image and depth.
 * 7. MASKS.  mask = the minimum of known over the 11 x 11 window clipped to the frame (BS:498; for a maximum or a minimum
 *    scipy's default `reflect` border is the same thing).  image = mask ? value : 0 (BS:497-499); depth is not masked.
 *    mask_hf (BS:501-503): with rr = min(r, H - 2), cc = min(c, W - 2),
 *    mask_hf[r][c] = |mask[rr][cc] - mask[rr + 1][cc]| + |mask[rr][cc] - mask[rr][cc + 1]| >= 1.
 *
 * ---- bsr_lift_pixels: the function ----
 * camera[21] = inverse of K (row-major), inverse of R (row-major), T: the caller inverts on the host in float64.
 * For pixel (r, c) with d = depth[r * W + c]:  a = ((float)c * d, (float)r * d, d) in fp32 (BS:470);
 *   cam[j] = (Kinv[j][0] a[0] + Kinv[j][1] a[1]) + Kinv[j][2] a[2] in fp64;  t[j] = cam[j] - T[j];
 *   point[j] = (float)((Rinv[j][0] t[0] + Rinv[j][1] t[1]) + Rinv[j][2] t[2]).
 * colour = image_f32[3 (r W + c) + k], or (float)image_u8[..] / 255.0f in fp32 (BS:472).
 * The selected pixels (select[r W + c] != 0; all of them for select == NULL) are written in row-major order, the order
 * of np.where at BS:545: output row = the number of selected pixels before this one.
 */
#ifndef BLOOMSCENE_REPROJECT_H_INCLUDED
#define BLOOMSCENE_REPROJECT_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_REPROJECT_SHIFT 28          /* S of step 4 */
#define BSR_REPROJECT_LIFT_BLOCK 256    /* pixels per count of bsr_lift_count */

/* Bytes of scratch bsr_warp_points needs: H * W * (5 * 8 + 4 + 1) -- the five sums, zmin, hit -- rounded up to 256.
 * 0 for an unsupported frame (H or W below 3, H * W of 2^31 or more). */
size_t bsr_reproject_scratch_bytes(int H, int W);

/*   P                          points, >= 0 (0: image, depth, mask, mask_hf are zeroed; no point pass is launched)
 *   points                     fp32, element k of point i at points[i * point_stride + k * comp_stride]: [P, 3] and [3, P]
 *                              are both read in place
 *   colors                     fp32 [P, 3] dense
 *   camera                     HOST, 21 doubles: K, R, T
 *   use_z_test, z_tolerance    steps 3 and 5; z_tolerance finite and >= 0, ignored when use_z_test is 0
 *   image [H, W, 3] fp32, depth [H, W] fp32, mask [H, W] uint8, mask_hf [H, W] uint8, pixel [P] int32: fully written
 *   scratch                    bsr_reproject_scratch_bytes(H, W) bytes, 8-byte aligned, contents ignored on entry (the call
 *                              clears it on the stream) */
int bsr_warp_points(int P, int H, int W, const float* points, long long point_stride, long long comp_stride,
                    const float* colors, const double* camera, int use_z_test, double z_tolerance, float* image,
                    float* depth, unsigned char* mask, unsigned char* mask_hf, int* pixel, void* scratch, void* hip_stream);

/* Bytes of scratch of the two lift calls with a selection: one uint32 count per BSR_REPROJECT_LIFT_BLOCK pixels, rounded up
 * to 256.  0 for H * W < 1 or >= 2^31. */
size_t bsr_lift_scratch_bytes(int H, int W);

/* Into the scratch: for every block b of 256 pixels, the number of selected pixels BEFORE pixel 256 b; *total (one uint32
 * on the device, fully written, which the caller reads once to size the outputs) = the number of all selected pixels. */
int bsr_lift_count(int H, int W, const unsigned char* select, void* scratch, unsigned* total, void* hip_stream);

/*   depth [H, W] fp32; exactly one of image_f, image_b ([H, W, 3] fp32 / uint8) is not NULL
 *   camera                     HOST, 21 doubles: inverse of K, inverse of R, T
 *   select                     [H, W] bytes or NULL (every pixel; scratch may then be NULL)
 *   scratch                    as bsr_lift_count left it for the same select
 *   n                          rows of the outputs: the count bsr_lift_count gave, H * W without a selection.  No row
 *                              at or beyond n is written, whatever the selection says
 *   points, colors             [n, 3] fp32 dense */
int bsr_lift_pixels(int H, int W, const float* depth, const float* image_f, const unsigned char* image_b,
                    const double* camera, const unsigned char* select, const void* scratch, int n, float* points,
                    float* colors, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
