// The layer-agnostic device functions of the row-per-lane MLP kernels (heads.hip, context.hip; anchor_state.hip takes the
// sigmoid): the products of a row with a weight matrix, the cooperative stores of whole rows, the activations.  What the
// row passes leave behind for the weight gradients is summed by mlp_wgrad.h.
//
// LANE MAPPING.  A lane is a row; a workgroup is ONE wave of 64 rows.  The row's vectors that are indexed by a loop
// variable live in LDS as [index][lane] with a pitch of 65 floats: the lane's own column is read without bank conflicts,
// and the cooperative, coalesced loads and stores of whole rows walk it with a stride of 65 (conflict-free as well).
// Eight outputs are accumulated at a time in registers; their weights are uniform over the wave: a block of 8 x 8 of them
// is one coalesced vector load, and each FMA takes its weight from a lane of it as a scalar operand (see THE WEIGHTS OF A
// STEP), with one LDS read per eight FMAs.  Every chain is written with explicit fmaf in the order the headers state: the
// build stays at -ffp-contract=off.
#pragma once
#include "common.h"

namespace bsr {

#define MLP_ROWS_T 64    // rows a workgroup (one wave)
#define MLP_ROWS_P 65    // LDS pitch of a [index][lane] vector
#define MLP_ROWS_NJ 8    // outputs accumulated at a time

// a load whose address is uniform over the wave (biases, the camera): through the scalar cache
typedef const float __attribute__((address_space(4))) mlp_cf;
__device__ __forceinline__ float uload(const float* p, int i) { return ((mlp_cf*)p)[i]; }
// lane `l` (a constant) of a wave-wide vector of weights, as a scalar operand
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ __forceinline__ float mlp_relu(float p) { return p > 0.0f ? p : (p != p ? p : 0.0f); }

__device__ __forceinline__ float mlp_tanh(float x)
{
	const float a = fabsf(x);
	float t;
	if (a < 0.25f) {
		const float u = a * a;
		t = a * (1.0f + u * (-1.0f / 3.0f + u * (2.0f / 15.0f + u * (-17.0f / 315.0f + u * (62.0f / 2835.0f)))));
	} else {
		const float e = bsr_expf(-2.0f * a);
		t = (1.0f - e) / (1.0f + e);
	}
	return copysignf(t, x);
}

__device__ __forceinline__ float mlp_sigmoid(float x) { return 1.0f / (1.0f + bsr_expf(-x)); }

// acc[j] = fmaf(x, weight in lane first + j * stride of wv, acc[j]) for the eight accumulators: the eight lane reads first,
// then eight independent FMAs (one scalar register reused read by read costs wait states between every pair)
__device__ __forceinline__ void step_fma(float x, float wv, int first, int stride, float* acc)
{
	float w[MLP_ROWS_NJ];
#pragma unroll
	for (int j = 0; j < MLP_ROWS_NJ; j++) w[j] = lane_value(wv, first + j * stride);
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int j = 0; j < MLP_ROWS_NJ; j++) acc[j] = fmaf(x, w[j], acc[j]);
	__builtin_amdgcn_sched_barrier(0);
}

// THE WEIGHTS OF A STEP.  A step of either product below is 8 x 8 weights: ONE coalesced vector load, lane l holding
// weight (l >> 3, l & 7) of the block, and the FMAs take them lane by lane as scalar operands (v_readlane).  The first
// build read them through the scalar cache instead; the 54 KB of weights stream through its 16 KB once per wave, and a
// wave waited on its misses for most of its life (docs/EXPERIMENTS.md).  The next step's load is issued before this
// step's FMAs.
//
// acc[jj] = the header's chain of output j0 + jj of the layer W [J, Kd], b [J] over in[k * MLP_ROWS_P], k ascending.
// Outputs past J repeat output J - 1 (never stored).
__device__ __forceinline__ void chain_rows(const float* __restrict__ W, const float* b, int J, int Kd, int j0, const float* in,
                                           float* acc, int lane)
{
#pragma unroll
	for (int jj = 0; jj < MLP_ROWS_NJ; jj++) acc[jj] = uload(b, j0 + jj < J ? j0 + jj : J - 1);
	const int jl = j0 + (lane >> 3) < J ? j0 + (lane >> 3) : J - 1, kl = lane & 7;
	const float* row = W + jl * Kd;
	float wv = row[kl < Kd ? kl : Kd - 1];
	int k = 0;
	for (; k + 8 <= Kd; k += 8) {
		const int kn = k + 8 + kl;
		const float wn = row[kn < Kd ? kn : Kd - 1];   // the next step's (or the tail's) weights
		float x[8];
#pragma unroll
		for (int i = 0; i < 8; i++) x[i] = in[(k + i) * MLP_ROWS_P];
#pragma unroll
		for (int i = 0; i < 8; i++) step_fma(x[i], wv, i, 8, acc);   // (k ascending per output: the header's order)
		wv = wn;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		if (k + i >= Kd) break;   // (uniform)
		const float x = in[(k + i) * MLP_ROWS_P];
		step_fma(x, wv, i, 8, acc);
	}
}

// acc[cc] = sum over r ascending of in[r * MLP_ROWS_P] * W[r][c0 + cc], W [R, C], from 0 with fmaf.  Indices past the
// matrix are clamped to its last element (columns past C are never stored, rows past R never used).
__device__ __forceinline__ void dot_cols(const float* __restrict__ W, int R, int C, int c0, const float* in, float* acc, int lane)
{
	const int last = R * C - 1, rl = lane >> 3, cl = c0 + (lane & 7);
#pragma unroll
	for (int cc = 0; cc < MLP_ROWS_NJ; cc++) acc[cc] = 0.0f;
	int at = rl * C + cl;
	float wv = W[at < last ? at : last];
	int r = 0;
	for (; r + 8 <= R; r += 8) {
		at = (r + 8 + rl) * C + cl;
		const float wn = W[at < last ? at : last];
		float x[8];
#pragma unroll
		for (int i = 0; i < 8; i++) x[i] = in[(r + i) * MLP_ROWS_P];
#pragma unroll
		for (int i = 0; i < 8; i++) step_fma(x[i], wv, i * 8, 1, acc);
		wv = wn;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		if (r + i >= R) break;   // (uniform)
		const float x = in[(r + i) * MLP_ROWS_P];
		step_fma(x, wv, i * 8, 1, acc);
	}
}

// dst[r * ld + c] = src[c * MLP_ROWS_P + r] for r < rows, c < C: consecutive lanes write consecutive columns of a row
// (`lane`, `threads`: the thread's index among the threads that store together, and their number)
__device__ __forceinline__ void coop_store(float* dst, size_t ld, int C, const float* src, int rows, int lane, int threads = MLP_ROWS_T)
{
	for (int idx = lane; idx < rows * C; idx += threads) {
		const int r = idx / C, c = idx - r * C;
		dst[(size_t)r * ld + c] = src[c * MLP_ROWS_P + r];
	}
}

// dst[r * ld + c] = 0 for r < rows, c < C: coop_store's walk
__device__ __forceinline__ void coop_zero(float* dst, size_t ld, int C, int rows, int lane, int threads = MLP_ROWS_T)
{
	for (int idx = lane; idx < rows * C; idx += threads) {
		const int r = idx / C, c = idx - r * C;
		dst[(size_t)r * ld + c] = 0.0f;
	}
}

// up to 8 values to the lane's own output row: two 16-byte stores (4-byte aligned) for a whole block
__device__ __forceinline__ void store_block(float* dst, const float* v, int count)
{
	if (count >= MLP_ROWS_NJ) {
		*reinterpret_cast<bsr_f32x4_a4*>(dst) = bsr_f32x4{v[0], v[1], v[2], v[3]};
		*reinterpret_cast<bsr_f32x4_a4*>(dst + 4) = bsr_f32x4{v[4], v[5], v[6], v[7]};
	} else {
#pragma unroll
		for (int i = 0; i < MLP_ROWS_NJ; i++)
			if (i < count) dst[i] = v[i];
	}
}

}  // namespace bsr
