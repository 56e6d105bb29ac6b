/*
 * bloomscene_voxelize.h -- C ABI of "quantise points to a voxel lattice and keep each voxel once", the operation that
 * decides which anchors exist in BloomScene's anchor model (scene/gaussian_model.py, "GM" below).  It occurs twice:
 *   anchor creation  GaussianModel.voxelize_sample, GM:435-438: np.unique(np.round(data / voxel_size), axis=0) * voxel_size
 *                    on the host, between the two distCUDA2 calls of create_from_pcd (GM:447, GM:464),
 *   anchor growing   GM:829-834: torch.round(x / cur_size).int() twice, a boolean gather of the [N * K, 3] tensor of
 *                    GM:824 and torch.unique(..., return_inverse=True, dim=0), three levels per adjust_anchor.
 *
 * Boundary rules are those of bloomscene_knn.h: plain DEVICE pointers and ints, a hipStream_t passed as void*,
 * 0 on success, bsr_last_error() on failure, no device allocation (all scratch comes from the caller), no state kept
 * between calls.  Nothing synchronises with the host: the calls can be captured into a hipGraph.  No float atomics (the
 * bounds are taken with integer atomics, which decide no result: a minimum does not depend on the order of its
 * operands).  Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION -- a pure function of the input, bit for bit and from run to run (tests/voxel_reference.py restates it
 * on the CPU).
 *
 * Input rows.  A call has E rows, numbered e in [0, E) ("positions").  Row e reads source row r(e) = rows ? rows[e] : e
 * of a source of P rows, in one of these forms:
 *   BSR_VOXEL_COORDS     src int32 [P, 3] dense: the coordinates themselves.  No rows list (E == P), no quantisation.
 *   BSR_VOXEL_POINTS_F   src fp32, BSR_VOXEL_POINTS_D src fp64: point r at src[r * src_stride + 0 .. 2] (src_stride in
 *                        ELEMENTS, >= 3: a column slice or a padded tensor is read in place).
 *   BSR_VOXEL_COMPOSITE  the flat offset list of GM:824: P = N * K, src = offset fp32 [N * K, 3] dense, and
 *                          x(r) = anchor[r / K] + src[r] * scaling[(r / K) * scaling_stride + 0 .. 2]
 *                        an fp32 multiply, then an fp32 add, each rounded, never fused.  anchor fp32 [N, 3] dense;
 *                        scaling is read through its row stride (get_scaling's [N, 6] is read in place).
 *   A rows entry outside [0, P) is never dereferenced; the row is INVALID.
 *
 * Quantisation (the point forms), per component x, with s = voxel_size converted to the points' type T:
 *   BSR_VOXEL_DIVIDE      q = rint(x / s) in T, the division correctly rounded.  numpy's GM:437 and torch's CPU kernels.
 *   BSR_VOXEL_RECIPROCAL  (fp32 only) q = rintf(x * (float)(1.0 / s)): the reciprocal is taken in DOUBLE from the double
 *                         voxel_size and rounded to fp32 once, then one fp32 multiply.  This is what torch's GPU kernel
 *                         computes for `tensor / python_scalar` (measured against torch 2.10: bit-equal quotients at six
 *                         voxel sizes on points within 2 ulp of the rounding boundaries; the reciprocal of the
 *                         fp32-rounded size, 1.0f / (float)s, is NOT it: 1 / 0.001 is 1000.0f the first way and
 *                         999.99994f the second), so what GM:829 / GM:832 compute in production.  The two rules put
 *                         some tens of every million points into different voxels.
 *   rint rounds ties to even; -0 is coordinate 0.  A row is INVALID if any q is not finite or lies outside
 *   [-2^31, 2^31).  (The reference's .int() of such a value is undefined; here it is counted and refused.)
 *
 * Invalid rows are counted on the device and never enter the sort: a call with at least one invalid row produces the
 * count and nothing else (U = 0, no output row is written).  bsr_voxel_quantise writes (0, 0, 0) for such a row.
 *
 * Result of bsr_voxel_unique, for the U distinct coordinate triples ("voxels") of the E rows:
 *   coords  int32 [U, 3]  the voxels in ascending lexicographic order of signed (x, y, z): the order of
 *                         np.unique(axis=0) and of torch.unique(dim=0), INT_MIN / INT_MAX included
 *   inverse int64 [E]     inverse[e] = the voxel number of row e
 *   first   int64 [U]     the smallest position e in the voxel (np.unique's return_index)
 *   counts  int64 [U]     the number of rows in the voxel
 *   points  [U, 3] of T, optional: T(c) * T(s) per component (GM:437's and GM:850's product; fp32 for the COORDS form
 *                         and the composite); a zero is always +0
 *   status  uint32 [8]    [0] U, [1] invalid rows, [2] key width in bits (bx + by + bz, up to 96), [3] refusal flags
 *                         (BSR_VOXEL_REFUSED_*), [4 .. 6] bx, by, bz, [7] 0
 * All outputs are sized for E rows by the caller; rows U .. E-1 are not written.
 *
 * Mechanism (csrc/voxelize.hip): quantise + per-axis bounds -> a 64-bit key per row holding (x - xmin, y - ymin,
 * z - zmin), each axis in exactly the bits its span needs, x highest (which keeps the lexicographic signed order), payload
 * the position -> a stable LSD radix sort on 8-bit digits (stability makes `first` the smallest position; passes above
 * the key width return at once and the width never travels to the host) -> head flags -> a fixed-order integer scan ->
 * emit.  Refusal: spans that need more than 64 bits together set BSR_VOXEL_REFUSED_WIDE, U = 0, no output row is
 * written; exactly 64 bits works.  (Real scenes need about 17 bits per axis.)
 *
 * Supported: 0 <= E < 2^31, 0 <= P < 2^31.  E == 0 launches nothing and writes nothing, the status included.
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_VOXELIZE_H_INCLUDED
#define BLOOMSCENE_VOXELIZE_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_VOXEL_COORDS    0
#define BSR_VOXEL_POINTS_F  1
#define BSR_VOXEL_POINTS_D  2
#define BSR_VOXEL_COMPOSITE 3

#define BSR_VOXEL_DIVIDE     0
#define BSR_VOXEL_RECIPROCAL 1

#define BSR_VOXEL_REFUSED_INVALID 1u   /* status[3]: at least one invalid row (status[1] counts them) */
#define BSR_VOXEL_REFUSED_WIDE    2u   /* status[3]: the three spans need more than 64 bits together */

/* Test-only, in the manner of BSR_FLAG_TEST_*: changes no result.  The sort's workgroups own 64 rows each instead of at
 * least 1024, so that inputs of a few thousand rows reach the many-workgroup code (more histogram columns than one step
 * of the row scan handles). */
#define BSR_VOXEL_FLAG_TEST_SMALL_CHUNK 0x100u

/* Step 1 alone: q[e] = the quantised coordinates of row e (the function above; (0, 0, 0) for an invalid row).  Replaces
 * torch.round(x / s).int() of GM:829 / GM:832.
 *   form     one of the three point forms; rule: BSR_VOXEL_DIVIDE or BSR_VOXEL_RECIPROCAL (fp32 forms only)
 *   src, src_stride, anchor, scaling, scaling_stride, K, rows: as above; anchor / scaling / K are read for the composite
 *            only, rows may be NULL (then E must equal P)
 *   q        int32 [E, 3], fully written
 *   invalid  uint32 [1] or NULL: the number of invalid rows (the call zeroes it on the stream first) */
int bsr_voxel_quantise(int form, int rule, int E, int P, const void* src, long long src_stride, const float* anchor,
                       const float* scaling, long long scaling_stride, int K, const long long* rows, double voxel_size,
                       int* q, unsigned int* invalid, void* stream);

/* Bytes of scratch bsr_voxel_unique needs for E rows (monotone in E; a multiple of 256; 0 for E <= 0).  Opaque to the
 * caller; need not be initialised.  About 36 E bytes: the quantised rows, two (key, payload) buffers, the histogram. */
size_t bsr_voxel_unique_scratch_bytes(int E);

/* The distinct voxels of the E rows (the function above).  Replaces np.unique(axis=0) of GM:437 and torch.unique(dim=0)
 * of GM:834 together with the quantisation and the gather in front of them.
 *   the source arguments: as for bsr_voxel_quantise, and form may be BSR_VOXEL_COORDS (rule and voxel_size are then used
 *            for `points` only)
 *   coords [E, 3] int32, inverse [E] int64, first [E] int64, counts [E] int64: the first U rows (inverse: all E) are
 *            written; points [E, 3] of T or NULL; status uint32 [8], fully written
 *   scratch  bsr_voxel_unique_scratch_bytes(E) bytes, 256-byte aligned, contents ignored on entry
 *   flags    0 or BSR_VOXEL_FLAG_TEST_SMALL_CHUNK */
int bsr_voxel_unique(int form, int rule, int E, int P, const void* src, long long src_stride, const float* anchor,
                     const float* scaling, long long scaling_stride, int K, const long long* rows, double voxel_size,
                     int* coords, long long* inverse, long long* first, long long* counts, void* points,
                     unsigned int* status, void* scratch, unsigned int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
