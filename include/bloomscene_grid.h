/*
 * bloomscene_grid.h -- C ABI of the deterministic multi-resolution hash-grid encoder that replaces BloomScene's
 * `_gridencoder` CUDA extension (submodules/gridencoder/src/gridencoder.cu, "GC" below) on the paths BloomScene calls:
 * grid_encode_forward / grid_encode_backward (GC:939-1000), from utils/encodings.py:230-349.
 *
 * Boundary rules are those of bloomscene_rast.h: plain DEVICE pointers and ints, a hipStream_t passed as void*,
 * 0 on success, bsr_last_error() on failure, no device allocation (the backward's scratch comes from the caller),
 * no state kept between calls.  Nothing synchronises with the host: both calls can be captured into a hipGraph.
 *
 * Layouts (dense row-major fp32 unless stated):
 *   inputs      [N, D]              coordinates; a point with a coordinate outside [0, 1] (or NaN) encodes to 0
 *   embeddings  [n_rows, F]         the whole table; aligned to min(16, 4 F) bytes
 *   offsets     [n_levels + 1] i32  ABSOLUTE first row of each computed level (a caller computing levels
 *                                   min_level .. min_level + n_levels - 1 passes a view starting at min_level);
 *                                   non-decreasing; hashmap_size of level l = offsets[l + 1] - offsets[l] > 0;
 *                                   offsets[n_levels] <= n_rows.  (Not in the reference: a corner whose level has
 *                                   no rows or whose row lies at or beyond n_rows is excluded like a border corner,
 *                                   so a malformed table cannot make the kernels reach outside the caller's buffers.)
 *   resolutions [n_levels] i32      >= 2
 *   outputs     [n_levels, N, F]    outputs[l][b][ch]
 *   dy_dx       [N, n_levels, D, F] dy_dx[b][l][d][ch]
 *   grad        [n_levels, N, F]    upstream gradient, layout of `outputs`
 * Supported: D in {1, 2, 3}, F in {1, 2, 4, 8} (the reference also has F = 16, 32: not supported here, error), 0 <=
 * n_levels <= 64, N * n_levels < 2^31.  The reference's `binary_vxl` and per-point `min_level_id` have no parameter:
 * they are not supported (the python layers raise NotImplementedError; there is no silent fall-back).
 *
 * Semantics per (point b, level l), restated from GC:100-663 with every fp32 operation in the reference's order
 * (tests/grid_reference.py restates them on the CPU; the forward is bit-equal to it, and tests/test_reference_grid_gpu.py
 * compares outputs, dy_dx and grad_inputs bit for bit with GC itself, compiled for gfx950 with -ffp-contract=off by
 * oracle/reference_build.py):
 *   pos = x * float(res - 2) + 0.5;  pg = floor(pos);  pos -= pg      (GC adds a DOUBLE 0.5 and narrows; here the add is
 *     fp32.  The same bits for every x in [0, 1]: the product is a non-negative fp32, so below 2^-25 both give 0.5, and
 *     from 2^-25 up its last bit is at 2^-48 or above, the sum fits 53 bits and the double add is exact: one rounding)
 *     DEVIATION FROM GC AS NVCC BUILDS IT: pos here is rounded twice (the product, then the sum), GC's source order.  A
 *     contracting compiler (nvcc's default; hipcc's too) narrows that add to fp32 and fuses it: pos = fma(x, float(res - 2),
 *     0.5), rounded once.  The two differ by an ulp of pos at some inputs, and where the source-order pos is an integer
 *     (x = (k + 0.5) / (res - 2) in fp32) floor() then picks the neighbouring cell: dy_dx, constant per cell, differs by whole
 *     row differences there, out by about ulp(pos) times its slope.  Documented, not matched (as with the knn FMA deviation);
 *     from pos on, a contracting build of GC and this library differ by rounding only (tests/test_reference_grid_gpu.py).
 *   corner c in 0 .. 2^D - 1: w = prod_d (bit d of c ? pos[d] : 1 - pos[d])  (d ascending),
 *     p[d] = bit d ? min(pg[d] + 1, res - 1) : pg[d];  a corner with some p[d] == 0 or p[d] == res - 1 is EXCLUDED
 *   wn = sum of the included w (c ascending), 1e-9 if it is 0;  wn_re = 1 / wn  (correctly rounded)
 *   row = dense index p[0] + p[1] res + p[2] res^2 while the stride stays <= hashmap_size, else
 *         p[0] ^ p[1] * 2654435761 ^ p[2] * 805459861 (uint32 wrap-around); either way % hashmap_size
 *   out[ch] = sum over included corners (c ascending) of (w * wn_re) * emb[offsets[l] + row][ch]
 *   dy_dx: the reference's formula GC:588-660, reproduced as written (edge weight float(res - 2) times the other
 *          dimensions' factors, excluded edge ends read 0, NOT renormalised by wn): the exact derivative of `out`
 *          only where every corner is included.
 */
#ifndef BLOOMSCENE_GRID_H_INCLUDED
#define BLOOMSCENE_GRID_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the scratch bsr_grid_encode_backward needs for a table of n_rows rows of n_features floats and n_levels
 * computed levels (monotone in each argument; a multiple of 256).  Opaque to the caller; need not be initialised. */
size_t bsr_grid_backward_scratch_bytes(int n_rows, int n_features, int n_levels);

/* Writes outputs [n_levels, N, F] and, when dy_dx is non-NULL, dy_dx [N, n_levels, D, F].  One launch.
 * Replaces grid_encode_forward (GC:939-967) -> kernel_grid (GC:100-663) with binary_vxl = min_level_id = NULL;
 * the reference's max_level, Rb and PV are unused there and have no parameter here.  N == 0 or n_levels == 0: no-op. */
int bsr_grid_encode_forward(int N, int num_dim, int n_features, int n_levels, int n_rows,
                            const float* inputs, const float* embeddings, const int* offsets, const int* resolutions,
                            float* outputs, float* dy_dx, void* stream);

/* Gradient of bsr_grid_encode_forward.  grad_embeddings [n_rows, F] is FULLY OVERWRITTEN (rows outside the computed
 * levels become 0; the reference adds into a tensor its caller zeroed, utils/encodings.py:301).  grad_inputs [N, D]
 * (optional; needs the forward's dy_dx) = sum over l, then ch, of grad[l][b][ch] * dy_dx[b][l][d][ch], in that order
 * (GC:864-891).  Replaces grid_encode_backward (GC:969-1000) -> kernel_grid_backward (GC:665-862) +
 * kernel_input_backward.
 *
 * DETERMINISTIC, NO FLOAT ATOMICS.  The reference scatters grad_embeddings with float atomicAdd (GC:850-856): its
 * result depends on arrival order.  Here every contribution is summed in 64-bit fixed point:
 *   G_l  = max |grad[l][b][ch]| over the FINITE values of level l (an integer max of the float bits: order-free)
 *   e_l  = the exponent with G_l < 2^e_l (frexp: normal G = 1.m 2^(E - 127) -> e = E - 126; subnormal -> bit length
 *          of the mantissa - 149);  k = ceil(log2 N) + D  (N 2^D bounds the contributions to one row)
 *   s_l  = min(61 - k - e_l, 126), or 0 when G_l == 0,  so that  N 2^D G_l 2^s_l < 2^61
 *   v    = (w * wn_re) * grad[l][b][ch]                  (fp32, the reference's order)
 *   q    = rint(ldexp(v, s_l)) as int64                  (round half to even; ldexp is exact)
 *   sum  = integer sum of q over the contributions to one (row, ch)   (integer atomics: associative)
 *   grad_embeddings[row][ch] = ldexp((float)sum, -s_l)   (one round-to-nearest int64 -> fp32 conversion)
 * The result is bit-identical on every run, stream and launch shape.  Error against the exact sum of the v:
 * 0.5 ulp of the result + count_row 2^(-s_l - 1), i.e. about 2^-39 G_l per contribution at N = 2^20, D = 3.
 * (Results in fp32's subnormal range are rounded a second time by the final ldexp.)
 * NON-FINITE INPUT: an element (row, ch) that receives a non-finite contribution (inf or NaN upstream gradient, or an
 * overflowing product) comes out NaN; every other element is unaffected.
 * scratch: bsr_grid_backward_scratch_bytes(n_rows, F, n_levels) bytes, 8-byte aligned, contents ignored.
 * N == 0 or n_levels == 0: grad_embeddings is zeroed, nothing else is written. */
int bsr_grid_encode_backward(int N, int num_dim, int n_features, int n_levels, int n_rows,
                             const float* grad, const float* inputs, const int* offsets, const int* resolutions,
                             const float* dy_dx, float* grad_embeddings, float* grad_inputs, void* scratch,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
