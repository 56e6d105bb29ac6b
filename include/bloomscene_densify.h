/*
 * bloomscene_densify.h -- C ABI of the two device steps of BloomScene's anchor densification
 * (GaussianModel.anchor_growing, scene/gaussian_model.py:807-895, "GM" below): the per-voxel feature maximum that GM:862
 * takes from the `torch_scatter` CUDA extension (`scatter_max`, imported at GM:22), and the test "is this candidate voxel
 * already occupied by an anchor" that GM:838-849 makes by comparing every candidate with every anchor.
 *
 * Boundary rules are those of bloomscene_knn.h: plain DEVICE pointers and ints, a hipStream_t passed as void*,
 * 0 on success, bsr_last_error() on failure, no device allocation (all scratch comes from the caller), no state kept
 * between calls.  Nothing synchronises with the host: the calls can be captured into a hipGraph.  No float atomics (the
 * maximum is taken on integers).  Purely additive: BSR_VERSION stays 4.
 *
 * bsr_scatter_max -- a pure function of the input, bit for bit (tests/densify_reference.py restates it on the CPU):
 *   contribution e in [0, E) reads source row r(e) = row_map ? row_map[e] : e and, for column f in [0, F), goes to group
 *   index(e, f) = index[e * is0 + f * is1].
 *   Ordering.    For a pair (g, f) the contributions are the e with index(e, f) == g.  They are ordered by the value
 *                src[r(e), f]: NaN is above everything (and all NaNs are equal), otherwise IEEE comparison, so -0 equals +0.
 *   Winner.      The smallest e among the maximal contributions.  out[g, f] = the winner's source bits verbatim (a -0
 *                stays -0, the first NaN keeps its payload); arg[g, f] = that e -- the contribution number, not r(e).
 *   Empty.       A pair without contributions gets out = +0.0 and arg = E (torch_scatter's documented convention).
 *   Out of range. A contribution whose row_map entry is outside [0, S) contributes to no column; an index entry outside
 *                [0, G) contributes nothing for that column.  Neither is dereferenced further, neither writes anything.
 *                (torch_scatter asserts on the device there.)
 *   Deviations.  torch_scatter's CUDA kernel leaves the argmax of tied maxima to a race between threads and its
 *                documentation is silent on NaN.  This function picks the deterministic answer: the first row wins (which
 *                is also its CPU path's answer) and NaN propagates like torch.amax.  The result is bit-identical from
 *                run to run.
 *
 * bsr_voxel_isin -- mask[u] = 1 where row u of query equals some row of keys in all three components, else 0: exact set
 * membership, whatever the coordinates (INT_MIN and INT_MAX included) and however often keys repeats a row.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_DENSIFY_H_INCLUDED
#define BLOOMSCENE_DENSIFY_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_VOXEL_MAX_KEYS (1 << 29)

/* out[g, f], arg[g, f] = the maximum over the contributions of group g in column f and the contribution it came from (the
 * function above).  Replaces torch_scatter.scatter_max(src, index, dim=0) of GM:862; with row_map it also replaces the
 * [N * n_offsets, feat_dim] tensor GM:861 repeats and masks only to feed that call (row_map[e] = the anchor of the e-th
 * selected offset).
 *   src      [S, F] fp32, dense row-major
 *   row_map  [E] int64, or NULL: then S must equal E and contribution e reads row e
 *   index    int64, element (e, f) at index[e * is0 + f * is1]; is0, is1 >= 0 are ELEMENT strides: (1, 0) is a 1-D index
 *            or an .expand(-1, F) view of one, (F, 1) a dense [E, F] index.  Nothing is copied.
 *   out      [G, F] fp32, arg [G, F] int64, 8-byte aligned: both fully written.  arg is also the call's working storage
 *            (a packed 64-bit (order key, inverted e) maximum is taken in it with integer atomics, then unpacked in
 *            place), so the call needs no scratch.  out and arg may not overlap the inputs.
 * Supported: 0 <= E < 2^31, 0 <= S < 2^31, 1 <= F, 0 <= G, G * F < 2^31.  G == 0 is a no-op; E == 0 writes the empty
 * result. */
int bsr_scatter_max(int E, int S, int F, int G, const float* src, const long long* row_map, const long long* index,
                    long long is0, long long is1, float* out, long long* arg, void* stream);

/* Bytes of scratch bsr_voxel_isin needs for N key rows (monotone in N; a multiple of 256; 0 for N <= 0 and for
 * N > BSR_VOXEL_MAX_KEYS).  Opaque to the caller: an open-addressing table of key row numbers, a power of two of at least
 * 2 N slots of 4 bytes. */
size_t bsr_voxel_isin_scratch_bytes(int N);

/* mask[u] = (query[u] is a row of keys), u in [0, U).  Replaces GM:838-849 before that code's negation
 * (`remove_duplicates`, U x 4096 x 3 booleans per chunk of anchors).
 *   query [U, 3] int32, keys [N, 3] int32, dense row-major; mask [U] uint8, fully written
 *   scratch: bsr_voxel_isin_scratch_bytes(N) bytes, 4-byte aligned; contents ignored on entry (the call clears what it
 *            needs on the stream)
 * Supported: 0 <= U, 0 <= N <= BSR_VOXEL_MAX_KEYS.  N == 0 gives all zeros; U == 0 is a no-op. */
int bsr_voxel_isin(int U, int N, const int* query, const int* keys, unsigned char* mask, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
