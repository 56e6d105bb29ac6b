// The integer prefix count over blocks that the compacting kernels share: a launch leaves one count per block of rows in
// an array, and a later launch's workgroup b needs the sum of the counts of the blocks before it -- always added in the
// same order, so a rank never depends on timing.  (anchor_state.hip's k_accum_apply spells the same steps out inline.)
#pragma once
#include "common.h"

namespace bsr {

#define BSR_COUNT_BLOCK 256
#define BSR_COUNT_WAVES (BSR_COUNT_BLOCK / 64)

// counts[0] + ... + counts[n - 1], the same on every thread.  Every thread of a BSR_COUNT_BLOCK workgroup calls it;
// `part` is BSR_COUNT_WAVES words of LDS that no other use shares until the next barrier after the call.
__device__ __forceinline__ uint32_t block_sum_counts(const uint32_t* __restrict__ counts, int n, uint32_t* part)
{
	uint32_t s = 0;
	for (int b = threadIdx.x; b < n; b += BSR_COUNT_BLOCK) s += counts[b];
	s = wave_inclusive_sum_dpp(s);
	if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = s;
	__syncthreads();
	uint32_t total = 0;
	for (int w = 0; w < BSR_COUNT_WAVES; w++) total += part[w];
	return total;
}

// The workgroup's own count of `p` over its threads, left in out[0] by thread 0.  `part`: as above.
__device__ __forceinline__ void block_store_count(uint32_t wave_count, uint32_t* part, uint32_t* out)
{
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_count;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t s = 0;
		for (int w = 0; w < BSR_COUNT_WAVES; w++) s += part[w];
		out[0] = s;
	}
}

}  // namespace bsr
