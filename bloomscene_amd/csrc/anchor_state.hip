// The two per-anchor blocks of a training iteration that the visible-anchor index list drives, for gfx950
// (include/bloomscene_anchor_state.h): the prologue of generate_neural_gaussians (gaussian_renderer/__init__.py:34-46)
// and GaussianModel.training_statis (scene/gaussian_model.py:742-759).
//
// A wave owns AST_ROWS consecutive rows and walks each tensor of those rows as ONE flat range of rows * C elements,
// element e on lane e % 64: consecutive lanes touch consecutive elements of a row, a dense output (or a dense
// gradient) is written as a contiguous block, and no lane idles on the narrow tensors (3, 6, K columns).  The row number
// of element e is e / C; the source row comes from the lane that loaded idx for it (one load per row, handed on with a
// lane read), so no LDS is used by A.
//   k_visible_fwd      AST_ROWS output rows a wave: the five gathers with their activations, then mask_anchor
//   k_visible_rate     one workgroup: the integer sum of the mask_anchor bytes, and the division
//   k_visible_bwd      AST_ROWS DENSE rows a wave.  idx is ascending, so the rows of the chunk [r0, r0 + rows) that are
//                      visible are idx[lo .. lo + m) with lo = lower_bound(idx, r0): one binary search a chunk, one load
//                      of up to AST_ROWS candidates, and a bit mask of the chunk's visible rows; row j's upstream row is
//                      lo + popcount(mask below j).  Every element of the dense gradients has exactly one writer, which
//                      writes the upstream or zero.
//   k_accum_count      a workgroup per scan block of BSR_ANCHOR_STATE_SCAN candidates: its number of selected
//                      candidates; and, a thread per visible anchor, opacity_accum and anchor_demon
//   k_accum_apply      a workgroup per scan block: the counts of the blocks before it (integer, fixed order), the rank
//                      of each of its selected candidates from wave ballots, and the two offset accumulators
// Nothing here dereferences an index it has not compared with the tensor's size first.
#include "common.h"
#include "mlp_rows.h"
#include "wg_scan.h"
#include "anchor_lattice.h"
#include "../../include/bloomscene_anchor_state.h"

namespace bsr {

#define AST_BLOCK 256
#define AST_WAVES (AST_BLOCK / 64)
#define AST_ROWS 16                        // rows a wave (<= 32: the backward's row mask is one word)
#define AST_SCAN BSR_ANCHOR_STATE_SCAN
#define AST_ROUNDS (AST_SCAN / AST_BLOCK)

// (quantize_anchor, rule A of the header: anchor_lattice.h, shared with the position coder)
__device__ __forceinline__ float mask_decision(float x) { return mlp_sigmoid(x) > 0.01f ? 1.0f : 0.0f; }

enum { AST_COPY, AST_ANCHOR, AST_EXP, AST_MASK };

// out[i0 .. i0 + rows)[C] from src rows `row_of` (lane j holds row j's source row, -1: none), through `Op`
template <int Op>
__device__ __forceinline__ void gather_rows(const float* __restrict__ src, size_t src_stride, int C, float* __restrict__ out,
                                            int i0, int rows, int row_of, int lane, const float* bmin, const float* bmax)
{
	float* o = out + (size_t)i0 * C;
	const int total = rows * C;
	for (int e = lane; e < total + 63 - (total + 63) % 64; e += 64) {   // (whole passes: every lane takes part in the lane read)
		const int j = (e < total ? e : total - 1) / C, c = (e < total ? e : total - 1) - j * C;
		const int r = __shfl(row_of, j);
		if (e >= total) continue;
		float v = 0.0f;
		if (r >= 0) {
			v = src[(size_t)r * src_stride + c];
			if (Op == AST_ANCHOR) v = quantize_anchor(v, bmin[c], bmax[c]);
			if (Op == AST_EXP) v = bsr_expf(v);
			if (Op == AST_MASK) v = mask_decision(v);
		}
		o[e] = v;
	}
}

__global__ void __launch_bounds__(AST_BLOCK) k_visible_fwd(int N, int n, int F, int K, const long long* __restrict__ idx,
                                                           const float* __restrict__ anchor, const float* __restrict__ bmin,
                                                           const float* __restrict__ bmax, const float* __restrict__ feat,
                                                           size_t feat_stride, const float* __restrict__ offset,
                                                           const float* __restrict__ scaling, const float* __restrict__ mask,
                                                           float* __restrict__ o_anchor, float* __restrict__ o_feat,
                                                           float* __restrict__ o_offsets, float* __restrict__ o_scaling,
                                                           float* __restrict__ o_masks, unsigned char* __restrict__ o_mask_anchor)
{
	const int lane = threadIdx.x & 63;
	const long long first = ((long long)blockIdx.x * AST_WAVES + (threadIdx.x >> 6)) * AST_ROWS;
	if (first >= (long long)n) return;   // (uniform over the wave)
	const int i0 = (int)first, rows = n - i0 < AST_ROWS ? n - i0 : AST_ROWS;
	int row_of = -1;
	if (lane < rows) {
		const long long r = idx[i0 + lane];
		if (r >= 0 && r < (long long)N) row_of = (int)r;
	}
	gather_rows<AST_COPY>(feat, feat_stride, F, o_feat, i0, rows, row_of, lane, nullptr, nullptr);
	gather_rows<AST_COPY>(offset, (size_t)3 * K, 3 * K, o_offsets, i0, rows, row_of, lane, nullptr, nullptr);
	gather_rows<AST_ANCHOR>(anchor, 3, 3, o_anchor, i0, rows, row_of, lane, bmin, bmax);
	gather_rows<AST_EXP>(scaling, 6, 6, o_scaling, i0, rows, row_of, lane, nullptr, nullptr);
	gather_rows<AST_MASK>(mask, (size_t)K, K, o_masks, i0, rows, row_of, lane, nullptr, nullptr);
	if (lane < rows) {
		bool any = false;
		if (row_of >= 0)
			for (int k = 0; k < K; k++) any = any || mask_decision(mask[(size_t)row_of * K + k]) != 0.0f;
		o_mask_anchor[i0 + lane] = any ? 1 : 0;
	}
}

// rate = fl32(number of non-zero bytes) / fl32(n).  flags is 4-byte aligned.
__global__ void __launch_bounds__(AST_BLOCK) k_visible_rate(int n, const unsigned char* __restrict__ flags, float* __restrict__ rate)
{
	__shared__ uint32_t wave_sum[AST_WAVES];
	const uint32_t* words = (const uint32_t*)flags;
	uint32_t count = 0;
	for (int w = threadIdx.x; w < n / 4; w += AST_BLOCK) count += __popc(words[w] & 0x01010101u);
	if ((int)threadIdx.x < n % 4) count += flags[n / 4 * 4 + threadIdx.x] & 1u;
	const uint32_t total = wg_total<AST_WAVES>(count, wave_sum);
	if (threadIdx.x == 0) rate[0] = (float)total / (float)n;   // (n == 0: 0 / 0)
}

enum { AST_G_COPY, AST_G_EXP, AST_G_MASK };

// d[r0 .. r0 + rows)[C] = the upstream row lo + (visible rows of the chunk below j), or 0
template <int Op>
__device__ __forceinline__ void scatter_rows(const float* __restrict__ g, int C, float* __restrict__ d, int r0, int rows,
                                             uint32_t visible, int lo, int lane, const float* __restrict__ aux)
{
	if (!d) return;
	float* o = d + (size_t)r0 * C;
	const int total = rows * C;
	for (int e = lane; e < total; e += 64) {
		const int j = e / C, c = e - j * C;
		float v = 0.0f;
		if (g && ((visible >> j) & 1u)) {
			const size_t i = (size_t)lo + __popc(visible & ((1u << j) - 1u));
			v = g[i * C + c];
			if (Op == AST_G_EXP) v = v * aux[i * C + c];
			if (Op == AST_G_MASK) {
				const float s = mlp_sigmoid(aux[(size_t)(r0 + j) * C + c]);
				v = (v * s) * (1.0f - s);
			}
		}
		o[e] = v;
	}
}

__global__ void __launch_bounds__(AST_BLOCK) k_visible_bwd(int N, int n, int F, int K, const long long* __restrict__ idx,
                                                           const float* __restrict__ mask, const float* __restrict__ grid_scaling,
                                                           const float* __restrict__ g_anchor, const float* __restrict__ g_feat,
                                                           const float* __restrict__ g_offsets, const float* __restrict__ g_scaling,
                                                           const float* __restrict__ g_masks, float* __restrict__ d_anchor,
                                                           float* __restrict__ d_feat, float* __restrict__ d_offset,
                                                           float* __restrict__ d_scaling, float* __restrict__ d_mask)
{
	const int lane = threadIdx.x & 63;
	const long long first = ((long long)blockIdx.x * AST_WAVES + (threadIdx.x >> 6)) * AST_ROWS;
	if (first >= (long long)N) return;   // (uniform over the wave)
	const int r0 = (int)first, rows = N - r0 < AST_ROWS ? N - r0 : AST_ROWS;
	int lo = 0, hi = n;                  // lower_bound(idx, r0): the same on every lane
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (idx[mid] < (long long)r0) lo = mid + 1; else hi = mid;
	}
	uint32_t visible = 0;
	if (lane < AST_ROWS && lo + lane < n) {
		const long long v = idx[lo + lane];
		if (v >= (long long)r0 && v < (long long)(r0 + rows)) visible = 1u << (int)(v - r0);
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) visible |= (uint32_t)__shfl_xor((int)visible, o);
	// (visible has at most as many bits as lanes that found one, all below n - lo: lo + a popcount stays inside idx's rows)
	scatter_rows<AST_G_COPY>(g_feat, F, d_feat, r0, rows, visible, lo, lane, nullptr);
	scatter_rows<AST_G_COPY>(g_offsets, 3 * K, d_offset, r0, rows, visible, lo, lane, nullptr);
	scatter_rows<AST_G_COPY>(g_anchor, 3, d_anchor, r0, rows, visible, lo, lane, nullptr);
	scatter_rows<AST_G_EXP>(g_scaling, 6, d_scaling, r0, rows, visible, lo, lane, grid_scaling);
	scatter_rows<AST_G_MASK>(g_masks, K, d_mask, r0, rows, visible, lo, lane, mask);
}

// ---- B ----

__global__ void __launch_bounds__(AST_BLOCK) k_accum_count(int N, int n, int K, const long long* __restrict__ idx,
                                                           const float* __restrict__ opacity,
                                                           const unsigned char* __restrict__ selection,
                                                           float* opacity_accum, float* anchor_demon,
                                                           uint32_t* __restrict__ counts)
{
	__shared__ uint32_t wave_sum[AST_WAVES];
	const int total = n * K;
	uint32_t count = 0;
#pragma unroll
	for (int q = 0; q < AST_ROUNDS; q++) {
		const long long c = (long long)blockIdx.x * AST_SCAN + q * AST_BLOCK + threadIdx.x;
		const bool s = c < (long long)total && selection[c] != 0;
		count += s ? 1u : 0u;
	}
	count = wg_total<AST_WAVES>(count, wave_sum);
	if (threadIdx.x == 0) counts[blockIdx.x] = count;
	for (long long i = (long long)blockIdx.x * AST_BLOCK + threadIdx.x; i < (long long)n; i += (long long)gridDim.x * AST_BLOCK) {
		const long long r = idx[i];
		if (r < 0 || r >= (long long)N) continue;
		float a = 0.0f;
		for (int k = 0; k < K; k++) {
			const float o = opacity[i * K + k];
			a = a + (o < 0.0f ? 0.0f : o);
		}
		opacity_accum[r] = opacity_accum[r] + a;
		anchor_demon[r] = anchor_demon[r] + 1.0f;
	}
}

__global__ void __launch_bounds__(AST_BLOCK) k_accum_apply(int N, int n, int K, int M, const long long* __restrict__ idx,
                                                           const unsigned char* __restrict__ selection,
                                                           const int* __restrict__ radii, const unsigned char* __restrict__ keep,
                                                           const float* __restrict__ grad, const uint32_t* __restrict__ counts,
                                                           float* offset_gradient_accum, float* offset_denom)
{
	__shared__ uint32_t before[AST_WAVES];
	__shared__ uint32_t wave_count[AST_ROUNDS][AST_WAVES];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int total = n * K;
	uint32_t rank = wg_total_of<AST_WAVES>(counts, (int)blockIdx.x, before);   // of the first candidate of this wave in round q
	bool sel[AST_ROUNDS];
	uint32_t below[AST_ROUNDS];
#pragma unroll
	for (int q = 0; q < AST_ROUNDS; q++) {
		const long long c = (long long)blockIdx.x * AST_SCAN + q * AST_BLOCK + threadIdx.x;
		sel[q] = c < (long long)total && selection[c] != 0;
		const uint64_t votes = wave_ballot(sel[q]);
		below[q] = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
		if (lane == 0) wave_count[q][wave] = (uint32_t)__popcll(votes);
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < AST_ROUNDS; q++) {
		for (int w = 0; w < AST_WAVES; w++) {
			if (w < wave) rank += wave_count[q][w];
		}
		if (sel[q]) {
			const uint32_t j = rank + below[q];
			if (j < (uint32_t)M && (keep ? keep[j] != 0 : radii[j] > 0)) {
				const int c = (int)((long long)blockIdx.x * AST_SCAN + q * AST_BLOCK + threadIdx.x);
				const int i = c / K, k = c - i * K;
				const long long r = idx[i];
				if (r >= 0 && r < (long long)N) {
					const float gx = grad[(size_t)j * 3], gy = grad[(size_t)j * 3 + 1];
					const size_t t = (size_t)r * K + k;
					offset_gradient_accum[t] = offset_gradient_accum[t] + sqrtf(gx * gx + gy * gy);
					offset_denom[t] = offset_denom[t] + 1.0f;
				}
			}
		}
		for (int w = 0; w < AST_WAVES; w++) {
			if (w >= wave) rank += wave_count[q][w];
		}
	}
}

static const char* check_sizes(int N, int n, int F, int K)
{
	if (N < 0) return "N must be >= 0";
	if (n < 0 || n > N) return "n must be in [0, N]";
	if (F < 1 || F > BSR_ANCHOR_STATE_MAX_F) return "F must be in [1, 64]";
	if (K < 1 || K > BSR_ANCHOR_STATE_MAX_K) return "K must be in [1, 16]";
	if ((long long)N * (F > 3 * K ? F : 3 * K) >= 0x80000000LL) return "N * max(F, 3 K) must be below 2^31";
	return nullptr;
}

static unsigned wave_chunks_grid(int rows) { return (unsigned)(((long long)rows + AST_ROWS * AST_WAVES - 1) / (AST_ROWS * AST_WAVES)); }

}  // namespace bsr

using namespace bsr;

extern "C" {

int bsr_anchor_visible_forward(int N, int n, int F, int K, const long long* idx, const float* anchor, const float* bound_min,
                               const float* bound_max, const float* feat, long long feat_stride, const float* offset,
                               const float* scaling, const float* mask, float* out_anchor, float* out_feat,
                               float* out_offsets, float* out_scaling, float* out_masks, unsigned char* out_mask_anchor,
                               float* out_rate, void* stream)
{
	const char* who = "bsr_anchor_visible_forward";
	if (const char* bad = check_sizes(N, n, F, K)) return fail("%s: %s (got N = %d, n = %d, F = %d, K = %d)", who, bad, N, n, F, K);
	if (feat_stride < (long long)F) return fail("%s: feat_stride must be >= F (got %lld, F = %d)", who, feat_stride, F);
	if (!out_rate) return fail("%s: NULL out_rate", who);
	if (n > 0) {
		if (!idx) return fail("%s: NULL idx", who);
		if (!anchor || !bound_min || !bound_max || !feat || !offset || !scaling || !mask) return fail("%s: NULL input", who);
		if (!out_anchor || !out_feat || !out_offsets || !out_scaling || !out_masks || !out_mask_anchor)
			return fail("%s: NULL output", who);
		if ((uintptr_t)out_mask_anchor & 3) return fail("%s: out_mask_anchor must be 4-byte aligned", who);
		if ((uintptr_t)idx & 7) return fail("%s: idx must be 8-byte aligned", who);
	}
	hipStream_t st = (hipStream_t)stream;
	if (n > 0)
		hipLaunchKernelGGL(k_visible_fwd, dim3(wave_chunks_grid(n)), dim3(AST_BLOCK), 0, st, N, n, F, K, idx, anchor, bound_min,
		                   bound_max, feat, (size_t)feat_stride, offset, scaling, mask, out_anchor, out_feat, out_offsets,
		                   out_scaling, out_masks, out_mask_anchor);
	hipLaunchKernelGGL(k_visible_rate, dim3(1), dim3(AST_BLOCK), 0, st, n, (const unsigned char*)out_mask_anchor, out_rate);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_anchor_visible_backward(int N, int n, int F, int K, const long long* idx, const float* mask,
                                const float* grid_scaling, const float* g_anchor, const float* g_feat,
                                const float* g_offsets, const float* g_scaling, const float* g_masks, float* d_anchor,
                                float* d_feat, float* d_offset, float* d_scaling, float* d_mask, void* stream)
{
	const char* who = "bsr_anchor_visible_backward";
	if (const char* bad = check_sizes(N, n, F, K)) return fail("%s: %s (got N = %d, n = %d, F = %d, K = %d)", who, bad, N, n, F, K);
	if (N == 0 || (!d_anchor && !d_feat && !d_offset && !d_scaling && !d_mask)) return 0;
	if (n > 0 && !idx) return fail("%s: NULL idx", who);
	if ((uintptr_t)idx & 7) return fail("%s: idx must be 8-byte aligned", who);
	if (n > 0 && d_scaling && g_scaling && !grid_scaling) return fail("%s: d_scaling needs grid_scaling", who);
	if (n > 0 && d_mask && g_masks && !mask) return fail("%s: d_mask needs mask", who);
	hipLaunchKernelGGL(k_visible_bwd, dim3(wave_chunks_grid(N)), dim3(AST_BLOCK), 0, (hipStream_t)stream, N, n, F, K, idx, mask,
	                   grid_scaling, g_anchor, g_feat, g_offsets, g_scaling, g_masks, d_anchor, d_feat, d_offset, d_scaling,
	                   d_mask);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

size_t bsr_anchor_accumulate_scratch_bytes(int n, int K)
{
	if (n <= 0 || K < 1 || K > BSR_ANCHOR_STATE_MAX_K || (long long)n * 3 * K >= 0x80000000LL) return 0;
	const size_t blocks = ((size_t)n * K + AST_SCAN - 1) / AST_SCAN;
	return align_up(blocks * sizeof(uint32_t), 256);
}

int bsr_anchor_accumulate(int N, int n, int K, int M, const long long* idx, const float* neural_opacity,
                          const unsigned char* selection, const void* filter, int filter_is_bool, const float* grad,
                          float* opacity_accum, float* anchor_demon, float* offset_gradient_accum, float* offset_denom,
                          void* scratch, void* stream)
{
	const char* who = "bsr_anchor_accumulate";
	if (const char* bad = check_sizes(N, n, 1, K)) return fail("%s: %s (got N = %d, n = %d, K = %d)", who, bad, N, n, K);
	if (M < 0) return fail("%s: M must be >= 0 (got %d)", who, M);
	if (n == 0) return 0;
	if (!idx) return fail("%s: NULL idx", who);
	if (!neural_opacity || !selection) return fail("%s: NULL input", who);
	if (M > 0 && (!filter || !grad)) return fail("%s: NULL filter or grad", who);
	if (!opacity_accum || !anchor_demon || !offset_gradient_accum || !offset_denom) return fail("%s: NULL accumulator", who);
	if (!scratch) return fail("%s: NULL scratch", who);
	if (((uintptr_t)scratch & 3) || ((uintptr_t)idx & 7) || (!filter_is_bool && ((uintptr_t)filter & 3)))
		return fail("%s: scratch and radii must be 4-byte, idx 8-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const unsigned blocks = (unsigned)(((size_t)n * K + AST_SCAN - 1) / AST_SCAN);
	uint32_t* counts = (uint32_t*)scratch;
	hipLaunchKernelGGL(k_accum_count, dim3(blocks), dim3(AST_BLOCK), 0, st, N, n, K, idx, neural_opacity, selection,
	                   opacity_accum, anchor_demon, counts);
	hipLaunchKernelGGL(k_accum_apply, dim3(blocks), dim3(AST_BLOCK), 0, st, N, n, K, M, idx, selection,
	                   filter_is_bool ? (const int*)nullptr : (const int*)filter,
	                   filter_is_bool ? (const unsigned char*)filter : (const unsigned char*)nullptr, grad,
	                   (const uint32_t*)counts, offset_gradient_accum, offset_denom);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
