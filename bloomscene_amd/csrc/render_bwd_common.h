// What the two backward walks share (k_render_bwd_strict: render_bwd_strict.hip; k_render_bwd_t: render_bwd.hip): the
// rows of the GAUSSIAN-MAJOR slab both write for k_preprocess_bwd, and the per-batch sum over the four quadrants.  A
// helper is here only if both kernels call it AND k_render_bwd_t compiles to the instructions it had with the text
// written out.  That decides the forms: scalars and pointers by value, no kernel local by reference ahead of the last
// use, no loop.  The per-pixel prologue and the walk-length reduction met it in no form tried (docs/EXPERIMENTS.md,
// "render_bwd.hip split") and stay written out in both kernels.
#pragma once
#include "tile_common.h"

namespace bsr {

// Index of this tile's instance of a Gaussian in the Gaussian-major order of KEPT instances (its
// block starts at inst_offset and enumerates the kept tiles of its rect row-major), from q3 / q2.w of
// the splat record.
__device__ __forceinline__ uint32_t instance_index(const uint32_t* __restrict__ wg_base, uint32_t id, const float4 q2,
                                                   const float4 q3, int tx, int ty)
{
	const uint32_t off = wg_base[id >> 8] + __float_as_uint(q3.x), lo = __float_as_uint(q3.y), wh = __float_as_uint(q3.z);
	const uint32_t xmin = lo & 0xffffu, ymin = lo >> 16, w = wh & 0xffffu, h = wh >> 16;
	const uint64_t mask = ((uint64_t)__float_as_uint(q2.w) << 32) | (uint64_t)__float_as_uint(q3.w);
	const uint32_t k = ((uint32_t)ty - ymin) * w + ((uint32_t)tx - xmin);
	return off + kept_rank(w * h, mask, k);
}

// Sum k of batch entry j over the four quadrants, in a fixed order -> deterministic; leaves the entry's partial sums zero
// for the next batch.
template <int NV, int ROW>
__device__ __forceinline__ float take_quadrant_sum(float (&part)[4][NV][ROW], const int k, const int j)
{
	const float a = ((part[0][k][j] + part[1][k][j]) + part[2][k][j]) + part[3][k][j];
	part[0][k][j] = 0.f;
	part[1][k][j] = 0.f;
	part[2][k][j] = 0.f;
	part[3][k][j] = 0.f;
	return a;
}

// One instance's row of the slab: 36 bytes, 40 with the depth gradient (rows are tight: 4-byte aligned).  The caller
// forms `row` itself: formed in here, the address arithmetic of both walks comes out differently.
template <bool DEPTH>
__device__ __forceinline__ void store_slab_row(float* const row, const float (&v)[10])
{
	*reinterpret_cast<bsr_f32x4_a4*>(row) = bsr_f32x4{v[0], v[1], v[2], v[3]};
	*reinterpret_cast<bsr_f32x4_a4*>(row + 4) = bsr_f32x4{v[4], v[5], v[6], v[7]};
	if (DEPTH) *reinterpret_cast<bsr_f32x2_a4*>(row + 8) = bsr_f32x2{v[8], v[9]};
	else row[8] = v[8];
}

// Entries no pixel of the tile reached (list positions n_walk .. n-1): zero rows, but they still need their map entry
template <bool DEPTH>
__device__ __forceinline__ void zero_unreached_rows(const int n_walk, const int n, const int tid, const uint32_t start,
                                                    const uint32_t* __restrict__ point_list, const uint32_t id_mask,
                                                    const float4* __restrict__ rec, const uint32_t* __restrict__ wg_base,
                                                    const int tx, const int ty, float4* __restrict__ slab)
{
	for (int pos = n_walk + tid; pos < n; pos += BSR_BLOCK) {
		const uint32_t slot = start + (uint32_t)pos;
		const uint32_t id = point_list[slot] & id_mask;
		const float zero[10] = {};
		float* const row = reinterpret_cast<float*>(slab) +
		                   (size_t)instance_index(wg_base, id, rec[(size_t)id * BSR_REC + 2], rec[(size_t)id * BSR_REC + 3],
		                                          tx, ty) * slab_row_floats(DEPTH);
		store_slab_row<DEPTH>(row, zero);
	}
}

}  // namespace bsr
