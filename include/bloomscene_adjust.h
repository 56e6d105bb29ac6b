/*
 * bloomscene_adjust.h -- C ABI of the anchor adjustment: GaussianModel.adjust_anchor (scene/gaussian_model.py:898-952,
 * "GM") with its callees anchor_growing (GM:807-895), cat_tensors_to_optimizer (GM:719-740) and
 * _prune_anchor_optimizer (GM:761-791), called every update_interval iterations at bloomscene.py:349.  The reference
 * decides with a dozen elementwise launches, appends every growth level to seven parameters, their moments and the
 * statistics with torch.cat, and then boolean-indexes all of them again.  What it computes is simple: each per-anchor
 * tensor of the result is the kept old rows in ascending order, followed by the new rows in level order.  Here that is
 *   A. bsr_adjust_decide   the decisions over the four statistics and the plan (which old row each kept row comes from)
 *   B. bsr_rows_resize     ONE launch that writes every new tensor (parameters, moments, statistics) exactly once
 * and the growth itself stays with include/bloomscene_voxelize.h and include/bloomscene_densify.h
 * (bloomscene_amd/adjust.py composes them).
 *
 * Boundary rules are those of bloomscene_rast.h: a hipStream_t passed as void*, 0 on success, bsr_last_error() on
 * failure, no state kept between calls.  The library allocates no device memory and waits for nothing on the host; both
 * calls can be captured into a hipGraph.  No float atomics (no atomics at all), bit-identical from run to run.  Purely
 * additive: BSR_VERSION stays 4.
 *
 * A. THE DECISIONS (GM:900-903, 811-812, 921-923).  N anchors, K offsets each, all statistics fp32.  Every comparison is
 * an fp32 comparison against a threshold that the caller forms in double (by the reference's own Python expression) and
 * the library rounds to fp32 ONCE, fl32(): what torch does for `tensor <op> python_scalar`.  A NaN compares false
 * everywhere.
 *   offset j in [0, N K):
 *     d  = offset_denom[j]
 *     q  = offset_gradient_accum[j] / d          correctly rounded; a NaN (0 / 0, a NaN statistic) becomes 0   GM:900-901
 *     g  = |q|                                    torch.norm over ONE element is |q| on the CPU, not sqrtf(q q):
 *                                                 3.3e-23 comes back unchanged there                            GM:902
 *     om = d > fl32(offset_count_min)             the caller passes check_interval * success_threshold * 0.5    GM:903
 *     offset_flags[j], one byte:  bit i (i < L) = g >= fl32(thresholds[i]) && om                               GM:811-812
 *                                 bit 7         = om
 *     thresholds is a HOST array of L doubles, 1 <= L <= 7; the caller fills it with
 *     threshold * ((update_hierachy_factor // 2) ** i)                                                          GM:810
 *   anchor r in [0, N):
 *     s = opacity_accum[r], d = anchor_demon[r]
 *     am    = d > fl32(anchor_count_min)          the caller passes check_interval * success_threshold          GM:922
 *     prune = s < fl(fl32(min_opacity) * d) && am                                                               GM:921, 923
 *     anchor_flags[r], one byte:  bit 0 = prune, bit 1 = am
 *   the plan:
 *     src_of[rank] = r (int32) for the rows with prune == 0, in ascending r; the entries from n_keep on are not written
 *     status (uint32 [4]) = { n_keep, number of anchors with am, number of offsets with om, 0 }
 *   The ranks are an integer prefix count in a fixed order: a count per block of BSR_ADJUST_SCAN rows, then every block
 *   adds the counts of the blocks before it.
 *   No deviation from torch on the GPU was found: the device's torch.norm over one element also returns 3.3e-23, 1e-30
 *   and 2e-19 unchanged (tests/test_adjust_gpu.py prints what it gives), and on statistics away from the thresholds the
 *   eager GM lines on the device decide as this does (the same test), so the device's division has shown no difference.
 *
 * B. THE RESIZE (GM:728-737, 769-787, 878-884, 908-947).  For every tensor of a HOST array of descriptors, read during
 * the call (the descriptors travel in the kernel-argument block, at most bsr_resize_max_tensors() per launch; more
 * tensors take more launches), with rows of `width` 4-byte elements whose BITS are moved (fp32 or int32):
 *     dst row i < n_keep       = src row src_of[i]; a src_of entry outside [0, N) is never dereferenced, its row is zeros
 *     dst row n_keep + a, a < A = append row a, or `fill` in every element when append == NULL
 *   op BSR_RESIZE_COPY          nothing else
 *   op BSR_RESIZE_ZERO_FLAGGED  a kept element whose flag byte has a bit of flag_mask is written as +0.  The flag byte of
 *                               element (r, c) of the SOURCE is flags[r] (flags_per_element == 0) or flags[r * width + c].
 *                               GM:908/914 is bit 7 of offset_flags per element on offset_denom and
 *                               offset_gradient_accum viewed as [N, K]; GM:938-939 is bit 1 of anchor_flags per row on
 *                               opacity_accum and anchor_demon.  Appended rows are not flagged.
 *   op BSR_RESIZE_CLAMP_FROM    an element v of a column >= clamp_col, kept OR appended, is written as
 *                               v > clamp ? clamp : v in fp32: a NaN stays, a value equal to the clamp stays.
 *                               GM:775-779 (_scaling[:, 3:] above 0.05 becomes 0.05) runs after the growth.
 *   Each output element is written exactly once, by one thread: a tensor whose width is a multiple of 4 and whose src,
 *   dst and append are 16-byte aligned moves in 16-byte pieces, any other element by element.  No LDS, no atomics.
 */
#ifndef BLOOMSCENE_ADJUST_H_INCLUDED
#define BLOOMSCENE_ADJUST_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_ADJUST_SCAN 1024         /* rows of one block of the prefix count */
#define BSR_ADJUST_MAX_K 16          /* offsets of an anchor */
#define BSR_ADJUST_MAX_LEVELS 7      /* thresholds of one call: bits 0 .. 6 of an offset's flag byte */
#define BSR_ADJUST_OFFSET_VALID 0x80 /* bit 7 of an offset's flag byte: om */
#define BSR_ADJUST_ANCHOR_PRUNE 0x01 /* bit 0 of an anchor's flag byte */
#define BSR_ADJUST_ANCHOR_VALID 0x02 /* bit 1 of an anchor's flag byte: am */

#define BSR_RESIZE_COPY 0
#define BSR_RESIZE_ZERO_FLAGGED 1
#define BSR_RESIZE_CLAMP_FROM 2
#define BSR_RESIZE_MAX_TENSORS 64   /* tensors of one launch: the descriptors fit HIP's 4 KB kernel-argument block */
#define BSR_RESIZE_MAX_WIDTH 1024
#define BSR_RESIZE_CHUNK 4096        /* output elements a workgroup writes */

/* Bytes of scratch bsr_adjust_decide needs for N anchors: a multiple of 256, monotone in N, 0 for N <= 0.  (Two counts
 * per block of BSR_ADJUST_SCAN anchors and one per block of as many offsets at BSR_ADJUST_MAX_K offsets an anchor.)  The
 * call writes every word of it that it reads: the scratch needs no initialisation. */
size_t bsr_adjust_decide_scratch_bytes(int N);

/* A.  All pointers but thresholds are DEVICE pointers: the four statistics [N], [N], [N K], [N K] fp32; offset_flags
 * [N K] and anchor_flags [N] bytes; src_of [N] int32; status [4] uint32; scratch of the size above, 4-byte aligned.
 * N == 0 launches nothing and writes nothing (the status of an empty model is the caller's four zeros).
 * Refused, before anything is launched: N < 0, K outside [1, BSR_ADJUST_MAX_K], N K >= 2^31, L outside
 * [1, BSR_ADJUST_MAX_LEVELS], NULL thresholds, a NaN among the thresholds or the three scalars, NULL status, and for
 * N > 0 a NULL statistic, a NULL output or a NULL or misaligned scratch. */
int bsr_adjust_decide(int N, int K, const float* opacity_accum, const float* anchor_demon,
                      const float* offset_gradient_accum, const float* offset_denom, int L, const double* thresholds,
                      double offset_count_min, double anchor_count_min, double min_opacity,
                      unsigned char* offset_flags, unsigned char* anchor_flags, int* src_of, unsigned int* status,
                      void* scratch, void* stream);

typedef struct bsr_resize_tensor {
	const void* src;             /* [N, width] dense, 4-byte elements (fp32 or int32: bits are moved) */
	void* dst;                   /* [n_keep + A, width] dense, FULLY written, must not overlap any src */
	const void* append;          /* [A, width] dense, or NULL: every appended element is `fill` */
	const unsigned char* flags;  /* NULL, or [N] bytes (per row) / [N * width] bytes (per element) */
	int width;                   /* 1 .. 1024 */
	int flags_per_element;
	unsigned int flag_mask;
	unsigned int fill;           /* bit pattern of an appended element when append == NULL */
	int op;                      /* BSR_RESIZE_COPY | BSR_RESIZE_ZERO_FLAGGED | BSR_RESIZE_CLAMP_FROM */
	int clamp_col;
	float clamp;                 /* CLAMP_FROM: columns >= clamp_col, v > clamp ? clamp : v */
} bsr_resize_tensor;

/* How many tensors one launch takes (BSR_RESIZE_MAX_TENSORS); bsr_rows_resize takes any number, in launches of this many. */
int bsr_resize_max_tensors(void);

/* B.  `tensors` is a HOST array; src, dst, append, flags and src_of ([n_keep] int32) are DEVICE pointers, 4-byte aligned.
 * n_tensors == 0, or n_keep + A == 0, launches nothing.
 * Refused, before anything is launched: n_tensors < 0 or a NULL array, N, n_keep or A negative, n_keep > N, NULL src_of
 * with n_keep > 0, and per tensor: width outside [1, BSR_RESIZE_MAX_WIDTH], an unknown op, (n_keep + A) * width >= 2^31,
 * NULL dst, NULL src with n_keep > 0, NULL flags with ZERO_FLAGGED and n_keep > 0, a flag_mask above 0xff, a clamp_col
 * outside [0, width], a pointer that is not 4-byte aligned, a dst that overlaps a src or an append of the call. */
int bsr_rows_resize(int n_tensors, const bsr_resize_tensor* tensors, int N, int n_keep, int A, const int* src_of, void* stream);

#ifdef __cplusplus
}
#endif
#endif
