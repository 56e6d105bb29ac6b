// The integer prefix sums and totals over ONE workgroup, stated once: over the workgroup's own lanes (one value or one
// predicate per thread) and over an array in global memory.  Integers: exact in any order, so nothing here decides a
// result -- only how many barriers and LDS round trips it costs.
//
// Conventions of every function below:
//   * WAVES is the workgroup's size in waves of 64 (blockDim.x == 64 * WAVES, one-dimensional); EVERY thread of the
//     workgroup calls the function, from uniform control flow (there is a barrier inside).
//   * The caller hands in the LDS (`s_wave`), so that a kernel calling in a loop can alternate two sets and keep ONE
//     barrier per step: a set may be handed in again once one other barrier of the workgroup lies behind the call (all
//     reads of it precede that barrier).  Functions that say "free on return" end with a barrier of their own.
//   * Wave sums are wave_inclusive_sum_dpp (common.h): vector ALU only, no ds_bpermute round trips.
#pragma once
#include "common.h"

namespace bsr {

// Exclusive sum of `v` over the workgroup's threads in thread order; `total` = the sum over all of them, on every thread.
// s_wave: WAVES words; one barrier.  (The digit bases of the radix scatters: thread d <-> digit d.)
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_sum(uint32_t v, uint32_t* s_wave, uint32_t& total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t incl = wave_inclusive_sum_dpp(v);
	if (lane == 63) s_wave[wave] = incl;
	__syncthreads();
	uint32_t before = 0u, all = 0u;
#pragma unroll
	for (int w = 0; w < WAVES; w++) {
		const uint32_t t = s_wave[w];
		before += w < wave ? t : 0u;
		all += t;
	}
	total = all;
	return before + incl - v;
}
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_sum(uint32_t v, uint32_t* s_wave)
{
	uint32_t total;
	return wg_exclusive_sum<WAVES>(v, s_wave, total);
}

// The same of a predicate: the number of threads before this one on which `p` holds (the rank of a compaction), and
// the number of all of them.  One ballot and two popcounts instead of the DPP sum.  s_wave: WAVES words; one barrier.
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_count(bool p, uint32_t* s_wave, uint32_t& total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t b = wave_ballot(p);
	if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
	__syncthreads();
	uint32_t before = 0u, all = 0u;
#pragma unroll
	for (int w = 0; w < WAVES; w++) {
		const uint32_t t = s_wave[w];
		before += w < wave ? t : 0u;
		all += t;
	}
	total = all;
	return before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_count(bool p, uint32_t* s_wave)
{
	uint32_t total;
	return wg_exclusive_count<WAVES>(p, s_wave, total);
}

// The sum of `v` over the workgroup's threads, on every thread.  s_wave: WAVES words; one barrier.
template <int WAVES>
__device__ __forceinline__ uint32_t wg_total(uint32_t v, uint32_t* s_wave)
{
	const uint32_t incl = wave_inclusive_sum_dpp(v);
	if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
	__syncthreads();
	uint32_t all = 0u;
#pragma unroll
	for (int w = 0; w < WAVES; w++) all += s_wave[w];
	return all;
}

// counts[0] + ... + counts[n - 1], on every thread: what the compacting kernels need of the per-block counts an earlier
// launch left -- workgroup b of the later launch asks for the blocks before it -- always added in the same order, so
// a rank never depends on timing.  s_wave: as wg_total.
template <int WAVES>
__device__ __forceinline__ uint32_t wg_total_of(const uint32_t* __restrict__ counts, int n, uint32_t* s_wave)
{
	uint32_t s = 0u;
	for (int b = threadIdx.x; b < n; b += 64 * WAVES) s += counts[b];
	return wg_total<WAVES>(s, s_wave);
}

// Exclusive scan of data[0 .. n) in place, VPT consecutive values per thread and step (64 * WAVES * VPT a step).
// Returns the total to every thread.  `write` false: the total alone, data untouched.  valid(i) false: element i is
// neither read nor counted (it is still overwritten with the running prefix: callers with holes never read them back).
// s_wave: 2 * WAVES words, two sets used in turn; free on return.
// One barrier per step: every thread adds up the wave totals itself (the carry lives in a register), and the
// totals of consecutive steps go to alternating sets, so that a step's writes are two barriers behind the last reads
// of the set they overwrite.  The next step's values are requested before this step's barrier.  (Until round 6 of
// the rasterizer: three barriers per step, the carry through LDS, a step beginning with the wait for its own loads -- a
// row of C5's pass-1 histogram is five steps long: k_scans 34 -> .. us.)
struct AllValid { __device__ __forceinline__ bool operator()(int) const { return true; } };
template <int WAVES, int VPT, typename Valid = AllValid>
__device__ __forceinline__ uint32_t wg_exclusive_scan(int n, uint32_t* data, uint32_t* s_wave, bool write, Valid valid = Valid())
{
	static_assert(VPT == 1 || VPT == 4 || VPT == 8, "the thread's own sum is written out for these");
	constexpr int STEP = 64 * WAVES * VPT;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t carry = 0u;
	uint32_t nx[VPT];
#pragma unroll
	for (int k = 0; k < VPT; k++) nx[k] = (tid * VPT + k < n && valid(tid * VPT + k)) ? data[tid * VPT + k] : 0u;
	int set = 0;
	for (int base = 0; base < n; base += STEP, set ^= WAVES) {
		const int i = base + tid * VPT;
		uint32_t v[VPT];
#pragma unroll
		for (int k = 0; k < VPT; k++) v[k] = nx[k];
#pragma unroll
		for (int k = 0; k < VPT; k++) nx[k] = (i + STEP + k < n && valid(i + STEP + k)) ? data[i + STEP + k] : 0u;
		// (written out per VPT: a loop, or a helper handed v, compiles k_scans' sum with two operands swapped -- the
		// same result, but tools/kernel_hashes.sh then reports the kernel as changed)
		uint32_t mine = v[0];
		if constexpr (VPT == 4) mine = v[0] + v[1] + v[2] + v[3];
		if constexpr (VPT == 8) mine = v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6] + v[7];
		const uint32_t incl = wave_inclusive_sum_dpp(mine);
		if (lane == 63) s_wave[set + wave] = incl;
		__syncthreads();
		uint32_t wave_off = 0u, total = 0u;
#pragma unroll
		for (int w = 0; w < WAVES; w++) {
			const uint32_t t = s_wave[set + w];
			wave_off += w < wave ? t : 0u;
			total += t;
		}
		uint32_t run = carry + wave_off + incl - mine;
		if (write) {
#pragma unroll
			for (int k = 0; k < VPT; k++) {
				if (i + k < n) data[i + k] = run;
				run += v[k];
			}
		}
		carry += total;
	}
	__syncthreads();   // (the caller may reuse s_wave at once)
	return carry;
}

}  // namespace bsr
