// The weight-gradient sums of the row-per-lane MLP units (heads.hip, context.hip), stated once (mlp_wgrad.hip).
//
// The reduction index of dW = dpre^T X is the row, which a unit's row pass has on the lane; so that pass leaves its per-row
// operands in the caller's scratch (MlpRowScratch: row-major, rows padded to 16 bytes) and two kernels add them up in the
// FIXED order the public headers promise, which depends on the shape alone:
//   k_mlp_wgrad   per range of MLP_WGRAD_CHUNK rows one partial of every weight-gradient element: a thread owns a 4 x 4
//                 block of one product and walks its range in row order, fp64 (a product of two fp32 values is exact
//                 there), rounded to fp32 once, when the partial is stored
//   k_mlp_wsum    adds the partials of an element in ascending range order, fp64, rounded to fp32 once
// A unit describes its stack with two tables that travel in the kernel-argument block: the PRODUCTS (what to multiply,
// and where in a partial the result goes) and the SEGMENTS (which piece of a partial is which gradient tensor of the
// caller).  The order of the segments is the element order of a partial.
#pragma once
#include "common.h"

namespace bsr {

#define MLP_WGRAD_CHUNK 256         // rows of a range: BSR_HEADS_CHUNK, BSR_CONTEXT_CHUNK
#define MLP_WGRAD_BLOCK 256
#define MLP_WGRAD_MAX_PRODUCTS 4    // the heads: W1 of the three heads stacked, W2 of each
#define MLP_WGRAD_MAX_SEGMENTS 12   // the heads: (W1, b1, W2, b2) x 3

// what a row pass leaves for the sums (all NULL: nothing is left): x [n, ldx], hid and dp1 [n, ldh], dp2 [n, ld2]
struct MlpRowScratch {
	float *x, *hid, *dp1, *dp2;
	size_t ldx, ldh, ld2;
};

struct MlpWgradLayout {
	size_t ldx, ldh, ld2;       // row pitches (floats): the width rounded up to a multiple of 4, + 4
	size_t chunks;              // ranges of MLP_WGRAD_CHUNK rows
	int tot;                    // weight-gradient elements
	size_t off_hid, off_dp1, off_dp2, off_partials, floats;
};

// x [n, wx], hid and dp1 [n, wh], dp2 [n, w2], `chunks` partials of `tot` elements, 64 floats
inline MlpWgradLayout mlp_wgrad_layout(int n, int wx, int wh, int w2, int tot)
{
	MlpWgradLayout l;
	l.ldx = (((size_t)wx + 3) & ~(size_t)3) + 4;
	l.ldh = (((size_t)wh + 3) & ~(size_t)3) + 4;
	l.ld2 = (((size_t)w2 + 3) & ~(size_t)3) + 4;
	l.chunks = ((size_t)n + MLP_WGRAD_CHUNK - 1) / MLP_WGRAD_CHUNK;
	l.tot = tot;
	l.off_hid = (size_t)n * l.ldx;
	l.off_dp1 = l.off_hid + (size_t)n * l.ldh;
	l.off_dp2 = l.off_dp1 + (size_t)n * l.ldh;
	l.off_partials = l.off_dp2 + (size_t)n * l.ld2;
	l.floats = l.off_partials + l.chunks * (size_t)l.tot + 64;
	return l;
}

// Contiguous pieces of a partial, in its element order, and the caller's tensor each one is summed into (NULL: not asked for).
struct MlpSegments {
	int count, tot;
	struct {
		int first, count;
		float* dst;
	} s[MLP_WGRAD_MAX_SEGMENTS];
	int add(int elements, float* dst)   // -> the segment's number
	{
		s[count] = {tot, elements, dst};
		tot += elements;
		return count++;
	}
};

// dW [J, Kd] = A^T B over the rows, db [J] = the column sums of A: row r of A is the J floats at A + r * lda, of B the Kd
// floats at B + r * ldb; dW (row-major) starts at element `out` of a partial, db at `bout`.  Units are numbered products
// in table order, each one's 4 x 4 blocks row blocks major; the blocks of the first column own the four bias sums.
struct MlpProduct {
	const float *A, *B;
	size_t lda, ldb;
	int J, Kd, out, bout;
};
struct MlpProducts {
	int count;
	MlpProduct p[MLP_WGRAD_MAX_PRODUCTS];   // (past count: zeros, a product without units)
	void add(const float* A, size_t lda, const float* B, size_t ldb, int J, int Kd, const MlpSegments& d, int w, int b)
	{
		p[count++] = {A, B, lda, ldb, J, Kd, d.s[w].first, d.s[b].first};
	}
};

// The host side of a backward entry point `who`, in the order it is called:
// any gradient asked for?  (false also for a table of NULLs)
bool mlp_wgrad_asked(const MlpSegments& d);
// refuses a destination that is not 4-byte aligned
int mlp_wgrad_check(const char* who, const MlpSegments& d);
// n == 0: every gradient asked for is zeros
int mlp_wgrad_zero(const char* who, const MlpSegments& d, hipStream_t st);
// the caller's scratch as the row pass sees it (left all NULL without `sums`); refuses a missing or misaligned one
int mlp_wgrad_carve(const char* who, const MlpWgradLayout& l, bool sums, void* scratch, MlpRowScratch& rs);
// after the row pass: the two launches
int mlp_wgrad_sums(const char* who, const MlpProducts& pr, const MlpSegments& d, int n, const MlpWgradLayout& l, void* scratch,
                   hipStream_t st);

}  // namespace bsr
