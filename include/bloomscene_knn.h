/*
 * bloomscene_knn.h -- C ABI of the mean squared distance to the three nearest neighbours that replaces BloomScene's
 * `simple_knn._C.distCUDA2` CUDA extension (submodules/simple-knn/simple_knn.cu, "SK" below: SimpleKNN::knn, SK:185-221,
 * with coord2Morton SK:63-76, boxMinMax SK:78-117, distBoxPoint / updateKBest / boxMeanDist SK:119-183), which
 * scene/gaussian_model.py:447 and :464 call to set the initial scale of every anchor.
 *
 * Boundary rules are those of bloomscene_rast.h: plain DEVICE pointers and ints, a hipStream_t passed as void*,
 * 0 on success, bsr_last_error() on failure, no device allocation (all scratch comes from the caller), no state kept
 * between calls.  Nothing synchronises with the host: the call can be captured into a hipGraph.  No float atomics.
 *
 * Semantics -- a pure function of the input, bit for bit (tests/knn_reference.py restates it on the CPU;
 * tests/test_reference_knn_gpu.py compares both with SK itself, compiled for gfx950 by oracle/reference_build.py):
 *   d(i, j)    = (dx*dx + dy*dy) + dz*dz,  dx = p_j.x - p_i.x etc.   fp32, every operation rounded, no contraction
 *   C(i)       = { d(i, j) : j != i, d(i, j) < FLT_MAX }   (NaN, inf and values >= FLT_MAX never count; duplicates
 *                                                          count, as 0)
 *   s0 <= s1 <= s2 = the three smallest values of C(i), padded with FLT_MAX
 *   out[i]     = ((s0 + s1) + s2) / 3.0f                  (correctly rounded division)
 * This is what SK's updateKBest keeps (a candidate enters only when `knn[j] > dist`, every slot starts at FLT_MAX), so
 * P = 1 and P = 2 give inf, P = 3 a finite value near 1.134e38, and a point with a NaN or infinite coordinate gets inf
 * and is nobody's neighbour.  SK's box pruning is exact, so its result does not depend on its Morton order, box size or
 * bounds (SK:193-198 starts the reduction at the origin); it is this function, except that nvcc contracts SK's
 * distance expressions into FMAs by default, which can move a result by a few ulp (as with the rasterizer's
 * libbsr_oracle_fma floor, this is documented, not matched).  That test asserts: bit-equal to SK compiled with
 * -ffp-contract=off; within a factor (1 + 2^-23)^6 (twelve roundings) of SK compiled with contraction.
 *
 * Supported: 0 <= P <= BSR_KNN_MAX_P.  P == 0 is a no-op.  (Entry point names carry no digits: the header / ctypes
 * table check of tests/test_host_cpu.py reads names as bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_KNN_H_INCLUDED
#define BLOOMSCENE_KNN_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_KNN_MAX_P (1 << 28)

/* Bytes of scratch bsr_knn_mean_dist needs for P points (monotone in P; a multiple of 256; 0 for P < 0).  Opaque to
 * the caller; need not be initialised.  About 40 P bytes. */
size_t bsr_knn_scratch_bytes(int P);

/* out[i] = the mean of the three smallest squared distances from point i to the other points (the function above).
 * points [P, 3] dense row-major fp32, 4-byte aligned; out [P] fp32, 4-byte aligned (fully written; may not overlap
 * points); scratch: bsr_knn_scratch_bytes(P) bytes, 16-byte aligned, contents ignored.  Replaces SimpleKNN::knn
 * (SK:185-221), which allocates, sorts with cub and reads the bounds back to the host twice. */
int bsr_knn_mean_dist(int P, const float* points, float* out, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
