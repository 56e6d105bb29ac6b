/*
 * bloomscene_mix_grid.h -- C ABI of the fused mixed 3D/2D binary hash-grid encoding: BloomScene's context encoding
 * pc.calc_interp_feat(anchor) (scene/gaussian_model.py:413-419, "GM" below) -- the normalisation by the anchor bounds,
 * mix_3D2D_encoding.forward (GM:98-105) over up to four GridEncoders (utils/encodings.py:351-435, "UE") and STE_binary
 * (UE:177-192) on their tables -- as ONE forward launch and one backward, without a materialised binary table.
 *
 * Boundary rules are those of bloomscene_rast.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (the backward's scratch comes from the caller), no state kept
 * between calls.  The arrays of length n_grids (params, offsets, resolutions, n_levels, n_rows, n_dims, dims,
 * grad_params) are HOST arrays, read during the call; what their pointer elements point to is device memory.  Nothing
 * synchronises with the host and nothing is read from the device on the host -- the bounds are device pointers -- so both
 * calls can be captured into a hipGraph.  No float atomics.  Purely additive: BSR_VERSION stays 4.
 *
 * INPUTS
 *   x [n, 3] fp32, row i at x + i * x_stride (a row stride in floats, >= 3; the column stride is 1): read in place.
 *   bound_min, bound_max: 3 device floats each, or both NULL.
 *   G = n_grids grids, 1 <= G <= 4.  Grid g:
 *     params[g] [n_rows[g], F]                   the table; aligned to min(16, 4 F) bytes
 *     offsets[g] [n_levels[g] + 1] i32, resolutions[g] [n_levels[g]] i32   device arrays with the meaning, and the
 *                                                malformed-table guards, of bloomscene_grid.h
 *     n_dims[g] = D_g in {1, 2, 3} and dims[3 g + k], k < D_g: distinct ascending indices into (x, y, z).  The mix of
 *                                                GM:98-104 is (0,1,2), (0,1), (0,2), (1,2) -- its chunk and three cats.
 *   F = n_features in {1, 2, 4, 8}, common to all grids.  L = sum of n_levels[g] <= 64.  n F L < 2^31, n >= 0.
 *   binary: a per-call flag.
 *
 * NORMALISATION (GM:417)
 *   u[d] = (x[d] - min[d]) / (max[d] - min[d]): an fp32 subtraction, an fp32 subtraction, then a correctly rounded
 *   division, in that order.  Without bounds u = x.
 *   DEVIATION: the reference's host assert of GM:416 (mean |x_bound_min| > 0, a device-to-host read) is gone.
 *
 * THE EMBEDDING VALUE READ AT A CORNER, p = params[g][row][ch]
 *   binary:     +1 where p >= 0 (this includes -0), -1 where p < 0, 0 where p is NaN -- STE_binary.forward (UE:181-185:
 *               both compares are false for a NaN, and the clamp changes no sign)
 *   not binary: p itself (UE:425, ste_binary = False without another quantiser)
 *   ste_multistep and add_noise (UE:420-423) are not implemented (the python layer raises NotImplementedError).
 *
 * PER (point b, grid g, level l): exactly the cell, corner exclusion, wn_re, row rule, interpolation and dy_dx formula
 * of bloomscene_grid.h, evaluated on u[dims[g]].  A point is "outside" (encodes to 0, gives and gets no gradient) per
 * grid, on that grid's own coordinates, as four separate calls would decide it.  The products w * (+-1) are exact, so
 * every result equals, bit for bit, bsr_grid_encode_forward on the materialised STE_binary table.
 *
 * OUTPUT
 *   out [n, C], C = F L, dense row-major: columns grid-major, then level, then channel -- the cat order of GM:104 over
 *   the reference's outputs.permute(1, 0, 2).reshape(N, L F) (UE:290).  Written once, in the layout the context head
 *   reads; there is no permute copy.
 *   dy_dx [n, W] (optional), W = F * sum of n_levels[g] D_g: per row, grid g's [n_levels[g], D_g, F] block
 *   (bloomscene_grid.h's dy_dx[b][l][d][ch]) at column F * sum over g' < g of n_levels[g'] D_g'.  Aligned to
 *   min(16, 4 F) bytes.  Written only when given.
 *
 * BACKWARD, for the upstream grad_out [n, C], row i at grad_out + i * grad_stride (>= C): read in place.
 *   grad_params[g] [n_rows[g], F] (NULL: the table is frozen and costs nothing) is FULLY OVERWRITTEN:
 *     the 64-bit fixed-point rule of bloomscene_grid.h per (grid, level), with N = n and D = D_g in s_l: the integer
 *     sums, and so the floats, are those of four separate bsr_grid_encode_backward calls.  With `binary` the result is
 *     multiplied by STE_binary's gate (UE:187-192): kept where |p| <= 1, +0 elsewhere; a NaN p gives +0 (the reference's
 *     grad * 0.0 gives -0 for a negative and NaN for a non-finite grad there).  The gate is applied in the pass that
 *     writes every element.  A non-finite contribution makes its element NaN where the gate is open, nothing else.
 *   grad_x [n, 3] dense (optional; needs the forward's dy_dx):
 *     r_g[d]    = bloomscene_grid.h's grad_inputs of grid g for its coordinate d, in its l-then-ch order from 0
 *     grad_u[d] = the sum of r_g[d] over the grids whose dims contain d, in ascending g, starting from the first such
 *                 grid's r_g[d] (0 when no grid selects d)
 *     grad_x[d] = grad_u[d] / (max[d] - min[d]), a correctly rounded division; grad_u[d] without bounds.
 *   The bounds get no gradient (the python layer refuses bounds that require one).
 *   The result is bit-identical from run to run.  ONE zero fill of the caller's scratch serves all grids.
 * n == 0 (or L == 0): the forward is a no-op; the backward zeroes every grad_params[g] given and writes nothing else.
 */
#ifndef BLOOMSCENE_MIX_GRID_H_INCLUDED
#define BLOOMSCENE_MIX_GRID_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_MIX_MAX_GRIDS 4

/* Bytes of the scratch bsr_mix_grid_backward needs: n_rows[g] (a HOST array of n_grids ints) is the rows of grid g, or 0
 * for a frozen grid, which takes no room; total_levels = the sum of n_levels over ALL grids.  A multiple of 256; opaque to
 * the caller; need not be initialised. */
size_t bsr_mix_grid_backward_scratch_bytes(int n_grids, const int* n_rows, int n_features, int total_levels);

/* Writes out [n, C] and, when dy_dx is non-NULL, dy_dx [n, W].  One launch. */
int bsr_mix_grid_forward(int N, int n_grids, int n_features, int binary, const float* x, long long x_stride,
                         const float* bound_min, const float* bound_max, const float* const* params,
                         const int* const* offsets, const int* const* resolutions, const int* n_levels, const int* n_rows,
                         const int* n_dims, const int* dims, float* out, float* dy_dx, void* stream);

/* The gradient of bsr_mix_grid_forward.  At most five launches: the zero fill of the scratch, the per-(grid, level)
 * max |grad|, the contribution pass, the finalize pass with the gate (these four only when some grad_params[g] is given,
 * and then scratch = bsr_mix_grid_backward_scratch_bytes(...) bytes, 8-byte aligned, contents ignored), and the input pass
 * (only when grad_x is given).  The zero fill is a kernel, not a memset: a captured backward holds kernel nodes only. */
int bsr_mix_grid_backward(int N, int n_grids, int n_features, int binary, const float* grad_out, long long grad_stride,
                          const float* x, long long x_stride, const float* bound_min, const float* bound_max,
                          const float* const* params, const int* const* offsets, const int* const* resolutions,
                          const int* n_levels, const int* n_rows, const int* n_dims, const int* dims, const float* dy_dx,
                          float* const* grad_params, float* grad_x, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
