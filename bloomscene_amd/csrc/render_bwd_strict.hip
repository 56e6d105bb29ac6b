// k_render_bwd_strict: the backward tile walk of BSR_FLAG_EXACT_GRAD (opt-in; every default frame runs k_render_bwd_t,
// render_bwd.hip).  Back-to-front re-traversal producing, per list entry (= per (tile, Gaussian) instance), the nine
// partial sums dL/d(mean2D.xy, conic.xyw, opacity, colour.rgb); semantics: reference renderCUDA (backward),
// cuda_rasterizer/backward.cu:399-586 of its depth-diff-gaussian-rasterization submodule.
//
// The reference's per-pair operations on the reference's operands (backward.cu:521,527-536,557,561-583): IEEE
// divisions, no fp contraction, the pinned exp on every pair, accum_rec channel by channel, the background term as a
// quotient and then a product (:557), the per-pair terms summed as they are -- only the ORDER of the nine sums then
// differs from the oracle's.  The pin is tests/test_strict_backward_gpu.py: under an upstream kept at ONE pixel every sum
// has at most one nonzero term and the nine accumulators equal the oracle's as values, DEPTH = false and DEPTH = true
// (zero depth upstream) alike; an operation changed in pair_terms_reference has to keep that test passing.  Until round
// 4 this walk (with the arithmetic shortcuts of k_render_bwd_t switched on one by one through attribution builds:
// docs/EXPERIMENTS.md) was also the default; ~2x the time of k_render_bwd_t.
//
// The reference issues 9 lane-scattered float atomicAdds per pair.  On MI355X lane-scattered
// global float atomics run ~17x below the contiguous rate (~20 G/s chip-wide), which would cap this
// kernel at ~2 ms for C3.  Instead NO global atomic is issued at all:
//   * the 9 partials are summed over the wave's 64 pixels by a halving reduction on lane-masked DPP
//     writes (bwd_sums.h: wave_sums_masked),
//   * each wave stores its sums in its own LDS slot (LDS float atomics cost ~16 cycles each on
//     gfx950 whatever the exec mask); the 4 slots are added in a fixed order at the batch end,
//   * each instance's 9 sums are written ONCE to its row [9 floats; 10 with the depth gradient] of a GAUSSIAN-MAJOR slab: the
//     rows of one Gaussian (one per kept tile of its rect, row-major) are adjacent, at the instance
//     numbering fixed by the forward's preprocess,
//   * k_preprocess_bwd later reads each Gaussian's rows as one contiguous run and adds them in that
//     fixed order.  (An earlier version wrote rows in list order and gathered them through an
//     instance->slot map: 48-B rows fetched at random cost 1.75 sectors each and the map another
//     scattered pass; moving the scatter to the write side made k_preprocess_bwd 23 % faster.)
// As in the forward pass, a 128-entry batch staged by waves 0 and 1 is first compacted per 8x8 quadrant
// (tile_common.h: stage_and_compact).
#include "bwd_sums.h"
#include "render_bwd_common.h"
#include "launch.h"

namespace bsr {

#define BSR_BWD_BATCH 128
// Row stride of the per-wave partial sums: the 9 (10) storing lanes of one entry write part[wave][k][j] for
// k = 0..NV-1 with ONE ds_write_b32 (bank = dword address mod 32, lanes of a 32-lane half conflict).  With rows of
// 128 floats all of them hit one bank; 129 puts component k on bank (k + j) mod 32.
#define BSR_BWD_ROW (BSR_BWD_BATCH + 1)
template <int NV>
struct BwdShared {
	TileStageT<BSR_BWD_BATCH> st;
	float part[4][NV][BSR_BWD_ROW];   // per-wave partial sums of the current batch (plain stores)
	uint32_t max_contrib[4];
};

// State a pixel carries along the list (back to front) and the constants of the pixel.
struct PairState {
	float T;
	float acc_rec[4], last_color[4], last_alpha;   // reference :527-536 channel by channel ([3] = depth, extension)
};
struct PixelConst {
	float dpx0, dpx1, dpx2, neg_T_final, bg_dot_dpixel, gz, g1, ddelx_dx, ddely_dy;
};
// Per pair the reference adds (:574-583), with dL_dG = o * dL_dalpha:
//   dL_dmean2D.x += dL_dG * dG_ddelx * ddelx_dx      dL_dconic.x += -0.5 gdx dx dL_dG
//   dL_dmean2D.y += dL_dG * dG_ddely * ddely_dy      dL_dconic.y += -0.5 gdx dy dL_dG
//   dL_dopacity  += G * dL_dalpha                    dL_dconic.w += -0.5 gdy dy dL_dG
// (source order: this translation unit is built with -ffp-contract=off)
template <bool DEPTH>
__device__ __forceinline__ void pair_terms_reference(PairState& st, const PixelConst& px, const float4 q0, const float4 q1,
                                                     const float4 q2, const float dx, const float dy, const float G,
                                                     const float alpha, float (&v)[10])
{
	const float om = 1.f - alpha;
	st.T = st.T / om;   // reference :521
	const float T = st.T;
	// accum_rec = last_alpha * last_color + (1 - last_alpha) * accum_rec, then (c - accum_rec) * dL_dpixel.  A pair the
	// reference skips must leave (accum_rec, last_color, last_alpha) standing.  The depth extension is the oracle's
	// separate pass (bsro_render_backward_depth): its own recurrence on d_i = gz z_i + g1.
	const bool live = G != 0.f;
	const float c4[4] = {q2.x, q2.y, q2.z, DEPTH ? px.gz * q1.w + px.g1 : 0.f};
	const float dp[3] = {px.dpx0, px.dpx1, px.dpx2};
	float S = 0.f, Sd = 0.f;
#pragma unroll
	for (int ch = 0; ch < (DEPTH ? 4 : 3); ch++) {
		const float ar = st.last_alpha * st.last_color[ch] + (1.f - st.last_alpha) * st.acc_rec[ch];
		st.acc_rec[ch] = live ? ar : st.acc_rec[ch];
		st.last_color[ch] = live ? c4[ch] : st.last_color[ch];
		if (ch < 3) S += (c4[ch] - st.acc_rec[ch]) * dp[ch];
		else Sd = c4[ch] - st.acc_rec[ch];
	}
	st.last_alpha = live ? alpha : st.last_alpha;
	// reference :557: a quotient, then a product ((-T_final * bg_dot) * (1 / om) rounds differently on ~40 % of pairs)
	const float dL_dalpha = T * S + (px.neg_T_final / om) * px.bg_dot_dpixel;
	const float ca = -2.0f * q0.z, cb = -q0.w, cc = -2.0f * q1.x;
	const float gdx = G * dx, gdy = G * dy;
	const float dG_ddelx = -gdx * ca - gdy * cb;
	const float dG_ddely = -gdy * cc - gdx * cb;
	float dL_dG = q1.z * dL_dalpha;
	v[0] = dL_dG * dG_ddelx * px.ddelx_dx;
	v[1] = dL_dG * dG_ddely * px.ddely_dy;
	v[2] = -0.5f * gdx * dx * dL_dG;
	v[3] = -0.5f * gdx * dy * dL_dG;
	v[4] = -0.5f * gdy * dy * dL_dG;
	v[5] = G * dL_dalpha;
	if (DEPTH) {   // the oracle's second pass: the same terms for dL_dalpha = T * (d_i - Rd)
		const float dLa = T * Sd;
		dL_dG = q1.z * dLa;
		v[0] += dL_dG * dG_ddelx * px.ddelx_dx;
		v[1] += dL_dG * dG_ddely * px.ddely_dy;
		v[2] += -0.5f * gdx * dx * dL_dG;
		v[3] += -0.5f * gdx * dy * dL_dG;
		v[4] += -0.5f * gdy * dy * dL_dG;
		v[5] += G * dLa;
	}
	const float aT = alpha * T;
	v[6] = aT * px.dpx0;
	v[7] = aT * px.dpx1;
	v[8] = aT * px.dpx2;
	v[9] = DEPTH ? aT * px.gz : 0.f;
}

// DEPTH = false: the reference's backward (dL_depths ignored).  DEPTH = true: the opt-in extension
// that also differentiates the normalised depth target (math in
// oracle/bsr_oracle.c:bsro_render_backward_depth): a tenth partial sum dL/dz per instance and one more
// term in dL/dalpha.  out_depth is the forward's depth image (its zeros are the acc <= 0.5 gate).
template <bool DEPTH>
__global__ void __launch_bounds__(BSR_BLOCK) k_render_bwd_strict(int n_tiles, int gx, int W, int H,
                                                                 const uint2* __restrict__ tile_range,
                                                                 const uint32_t* __restrict__ point_list,
                                                                 const float4* __restrict__ rec,
                                                                 const uint32_t* __restrict__ wg_base,
                                                                 const float* __restrict__ bg_color,
                                                                 const float* __restrict__ final_Ts,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const float* __restrict__ dL_dpixels,
                                                                 const float* __restrict__ out_depth,   // DEPTH only
                                                                 const float* __restrict__ dL_depths,   // DEPTH only
                                                                 const int* __restrict__ masks_flag,    // forward's hand-over word (flags[6]; flags[2] = kept instances)
                                                                 int capacity,                          // the R the call was handed
                                                                 float4* __restrict__ slab)        // [R][9 or 10 floats]
{
	constexpr int NV = DEPTH ? 10 : 9;
	__shared__ BwdShared<NV> sh;

	const int tile = xcd_tile(blockIdx.x, n_tiles);
	if (tile >= n_tiles) return;
	// more instances kept than the R this call was handed: an overflowed BSR_FLAG_NO_READBACK forward -- no lists exist
	// (k_preprocess_bwd writes NaN gradients, the thread's next forward reports it)
	if (__builtin_amdgcn_readfirstlane(masks_flag[-4]) > capacity) return;
	// (the per-pixel prologue, down to ddely_dy, is written out in both walks: render_bwd_common.h)
	const int tid = threadIdx.x;
	const int wave = tid >> 6, lane = tid & 63;
	const int tx = tile % gx, ty = tile / gx;
	const int px = tx * BSR_TILE + ((wave & 1) << 3) + (lane & 7);
	const int py = ty * BSR_TILE + ((wave >> 1) << 3) + (lane >> 3);
	const bool inside = px < W && py < H;
	const float pixfx = (float)px, pixfy = (float)py;
	const float tile_x0 = (float)(tx * BSR_TILE), tile_y0 = (float)(ty * BSR_TILE);
	const size_t pix_id = (size_t)W * py + px;
	const size_t plane = (size_t)H * W;

	const uint2 range = tile_range[tile];
	const uint32_t start = range.x;
	const int n = (int)(range.y - range.x);
	// (the forward may have left its box tests in the top byte of the point_list words: k_render_bwd_t; unused here)
	const uint32_t id_mask = __builtin_amdgcn_readfirstlane(*masks_flag) != 0 ? 0x00ffffffu : 0xffffffffu;

	const float T_final = inside ? final_Ts[pix_id] : 0.0f;
	PairState pst = {};
	pst.T = T_final;
	const uint32_t last_contributor = inside ? n_contrib[pix_id] : 0u;
	PixelConst pc = {};
	if (inside) {
		pc.dpx0 = dL_dpixels[pix_id];
		pc.dpx1 = dL_dpixels[plane + pix_id];
		pc.dpx2 = dL_dpixels[2 * plane + pix_id];
	}
	pc.bg_dot_dpixel = bg_color[0] * pc.dpx0 + bg_color[1] * pc.dpx1 + bg_color[2] * pc.dpx2;
	pc.neg_T_final = -T_final;
	// depth extension: d_i = gz * z_i + g1 plays the role of a fourth colour channel
	if (DEPTH && inside) {
		const float depth_px = out_depth[pix_id];
		if (depth_px != 0.0f) {   // the forward's acc > 0.5 decision
			pc.gz = dL_depths[pix_id] / (1e-6f + (1.0f - T_final));
			pc.g1 = -pc.gz * depth_px;
		}
	}
	// component whose wave total lands in this lane after the reduction; one lane per component stores
	bool stores;
	const int comp_of_lane = calibrate_components<DEPTH>(lane, stores);
	float* const part_mine = &sh.part[wave][stores ? comp_of_lane : 0][0];
	pc.ddelx_dx = (float)(0.5 * W);
	pc.ddely_dy = (float)(0.5 * H);

	// Entries at list positions >= max(last_contributor) are skipped by every pixel of the tile
	// (reference :498-500): start the walk at the deepest entry any pixel blended.
	// (written out in both walks: render_bwd_common.h)
	uint32_t m = last_contributor;
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
	if (lane == 0) sh.max_contrib[wave] = m;
	if (tid < BSR_BWD_BATCH) {
#pragma unroll
		for (int w = 0; w < 4; w++)
#pragma unroll
			for (int k = 0; k < NV; k++) sh.part[w][k][tid] = 0.f;
	}
	__syncthreads();
	const int n_walk = (int)max(max(sh.max_contrib[0], sh.max_contrib[1]), max(sh.max_contrib[2], sh.max_contrib[3]));

	for (int base = 0; base < n_walk; base += BSR_BWD_BATCH) {
		const int cnt = min(BSR_BWD_BATCH, n_walk - base);
		const int top = n_walk - 1 - base;   // list position of batch entry j is top - j
		const bool valid = tid < cnt;
		uint32_t my_row = 0;
		float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
		if (valid) {
			const uint32_t my_slot = start + (uint32_t)(top - tid);
			const uint32_t id = point_list[my_slot] & id_mask;
			const float4* r = rec + (size_t)id * BSR_REC;   // one 64-B line: record + rect + instance offset
			r0 = r[0];
			r1 = r[1];
			r2 = r[2];
			my_row = instance_index(wg_base, id, r2, r[3], tx, ty);   // the entry's row in the Gaussian-major slab
		}
		// (the trailing barrier of the previous iteration fenced the staging buffers)
		const int n_mine = stage_and_compact(sh.st, tid, valid, r0, r1, r2, tile_x0, tile_y0);
		const int n_u = __builtin_amdgcn_readfirstlane(n_mine);
		// entry j of the batch sits at list position top - j; this pixel blended positions < last_contributor
		// (reference :498-500): j > top - last_contributor, compared on the pre-scaled list offsets
		const int joff_min = (top - (int)last_contributor) * 16;
		auto visit = [&](const unsigned int joff) {
			const char* rec = stage_rec(sh.st, joff);
			const float4 q0 = rec_q0<BSR_BWD_BATCH>(rec);
			const float4 q1 = rec_q1<BSR_BWD_BATCH>(rec);   // conic c, power cut, opacity, depth
			const float dx = q0.x - pixfx;
			const float dy = q0.y - pixfy;
			const float power = (q0.z * dx * dx + q1.x * dy * dy) + q0.w * dx * dy;   // pre-scaled conic (common.h): the forward's bits
			const bool cand = ((int)joff > joff_min) && !(power > 0.0f) && !(power < q1.y);
			if (wave_ballot(cand) == 0ull) return;   // wave-uniform
			const float4 q2 = rec_q2<BSR_BWD_BATCH>(rec);
			// The forward decided `alpha >= 1/255` on alpha = min(0.99, o * E(power)) with the pinned exp E (bsr_expf) --
			// in its default mode only inside the decision band, outside of which every exp within ulps decides alike
			// (render_fwd.hip) -- and the backward must take the same decision on every pair (the T chain divides by the
			// same factors the forward multiplied).  Lanes that must not blend carry G = 0, hence alpha = 0: every
			// recurrence then leaves their state unchanged (T / 1 = T) and all nine contributions are exactly 0.
			float G = cand ? bsr_expf_walk(power) : 0.f;
			float alpha = fminf(0.99f, q1.z * G);
			const bool active = !(alpha < 1.0f / 255.0f);
			if (wave_ballot(active) == 0ull) return;
			G = active ? G : 0.f;
			alpha = active ? alpha : 0.f;
			float v[10];
			pair_terms_reference<DEPTH>(pst, pc, q0, q1, q2, dx, dy, G, alpha, v);
			const float tot = wave_sums_masked<DEPTH>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]);
			if (stores) *reinterpret_cast<float*>(reinterpret_cast<char*>(part_mine) + (joff >> 2)) = tot;   // part_mine[j]
		};
		// four list entries per trip: one address computation and one 16-byte LDS read for the list
		for (int i = 0; i < n_u; i += 4) {
			const uint4 l = *reinterpret_cast<const uint4*>(&sh.st.list[wave][i]);   // (reads past the end stay inside the list)
			visit(l.x);
			if (i + 1 < n_u) visit(l.y);
			if (i + 2 < n_u) visit(l.z);
			if (i + 3 < n_u) visit(l.w);
		}
		__syncthreads();
		if (valid) {
			float a9[10];
			a9[9] = 0.f;
#pragma unroll
			for (int k = 0; k < NV; k++) a9[k] = take_quadrant_sum(sh.part, k, tid);
			float* const row = reinterpret_cast<float*>(slab) + (size_t)my_row * slab_row_floats(DEPTH);
			store_slab_row<DEPTH>(row, a9);
		}
		__syncthreads();
	}

	zero_unreached_rows<DEPTH>(n_walk, n, tid, start, point_list, id_mask, rec, wg_base, tx, ty, slab);
}

template <bool DEPTH>
static void launch_strict(const RenderBwdArgs& a, hipStream_t s)
{
	const int n_tiles = a.gx * a.gy;
	const int blocks = ((n_tiles + 7) / 8) * 8;
	hipLaunchKernelGGL((k_render_bwd_strict<DEPTH>), dim3(blocks), dim3(BSR_BLOCK), occupancy_sweep_lds_pad("BSR_SWEEP_LDS_PAD_BWD"),
	                   s, n_tiles, a.gx, a.W, a.H, a.tile_range, a.point_list, a.rec, a.wg_base, a.bg, a.final_T, a.n_contrib,
	                   a.dL_dpix, DEPTH ? a.out_depth : nullptr, DEPTH ? a.dL_depths : nullptr, a.masks_flag, a.capacity, a.slab);
}

void launch_render_bwd_strict(const RenderBwdArgs& a, hipStream_t s)
{
	if (a.out_depth && a.dL_depths) launch_strict<true>(a, s);
	else launch_strict<false>(a, s);
}

}  // namespace bsr
