// The deterministic grid-wide fp64 sum of the loss kernels (photometric, entropy, depth prior), stated once.  Their
// public headers promise this ORDER, and with it results that are bit-identical from run to run for a given grid:
//   1. per wave a xor butterfly, offsets 32, 16, 8, 4, 2, 1 (every lane ends with the same bits: each step adds the same
//      two values on both sides);
//   2. the wave results added in wave order from the left -- ((s0 + s1) + s2) + s3 for four waves;
//   3. thread 0 stores the workgroup's partial; a fence and an integer ticket pick the last workgroup to arrive;
//   4. that workgroup re-reads all partials, thread t adding those of workgroups t, t + BLOCK, ... in that order, and
//      reduces once more by steps 1 and 2.
// No float atomics; the only atomic is the integer ticket, which the host zeroes before the launch.
#pragma once
#include "common.h"
#include <utility>

namespace bsr {

// ((s[0] + s[1]) + s[2]) + ... over the W wave results, as one expression (step 2): wave_order_sum(s, std::make_integer_sequence<int, W>())
template <int W, int... K>
__device__ __forceinline__ double wave_order_sum(const double (&s)[W], std::integer_sequence<int, K...>) { return (... + s[K]); }

// Relaxed agent-scope loads: what the last workgroup reads was written by other workgroups of the same launch, so it
// must come from memory, not from a line this CU cached before the ticket was drawn.
__device__ __forceinline__ double load_f64(const double* p)
{
	return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned load_u32(const unsigned* p)
{
	return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread 0 draws the workgroup's ticket (after its partial is stored) -> whether this workgroup is the last of the
// grid, to all threads.  Every thread of the workgroup calls it, whatever the block size; it brings its own word of
// LDS and opens with a barrier, so a second call in one kernel is safe.  In the last workgroup every partial that any
// workgroup stored before its own call is visible to load_f64 / load_u32 afterwards.
__device__ __forceinline__ bool grid_last_ticket(unsigned* ticket)
{
	__shared__ int s_last;
	__syncthreads();
	if (threadIdx.x == 0) {
		__threadfence();
		s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
	}
	__syncthreads();
	const bool last = s_last != 0;
	if (last) __threadfence();
	return last;
}

// The workgroup's sums v[0..N) -> its N partials in psum[N * blockIdx.x ..); the last workgroup to arrive adds the
// partials.  Returns true in thread 0 of that workgroup, with the totals in v.  Every thread of every workgroup of BLOCK
// threads must call it (a one-dimensional grid).  It brings its own LDS (N * BLOCK / 64 doubles) and leaves it behind
// a barrier: free for reuse on return.  psum: N * gridDim.x doubles.
template <int N, int BLOCK>
__device__ __forceinline__ bool grid_sum(double (&v)[N], unsigned* ticket, double* psum)
{
	static_assert(BLOCK % 64 == 0, "whole waves");
	__shared__ double s_w[N][BLOCK / 64];
	const int tid = threadIdx.x, wave = tid >> 6;
	for (int pass = 0; pass < 2; pass++) {
#pragma unroll
		for (int k = 0; k < N; k++)
			for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
		if ((tid & 63) == 0) {
#pragma unroll
			for (int k = 0; k < N; k++) s_w[k][wave] = v[k];
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < N; k++) v[k] = wave_order_sum(s_w[k], std::make_integer_sequence<int, BLOCK / 64>());
		__syncthreads();
		if (pass == 1) return tid == 0;
		if (tid == 0) {
#pragma unroll
			for (int k = 0; k < N; k++) psum[N * (size_t)blockIdx.x + k] = v[k];
		}
		if (!grid_last_ticket(ticket)) return false;
#pragma unroll
		for (int k = 0; k < N; k++) v[k] = 0.0;
		for (unsigned b = tid; b < gridDim.x; b += BLOCK)
#pragma unroll
			for (int k = 0; k < N; k++) v[k] += load_f64(&psum[N * (size_t)b + k]);
	}
	return false;
}

}  // namespace bsr
