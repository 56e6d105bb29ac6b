// Multi-resolution hash-grid encoder for gfx950 (include/bloomscene_grid.h): BloomScene's `_gridencoder`
// grid_encode_forward / grid_encode_backward, restated from gridencoder.cu ("GC") with a deterministic backward.
//
// Launch shape: one thread per (point b, level l), flattened level-major (t = l * N + b): a wave shares one level
// (its offset, resolution, hashmap size and dense-or-hashed choice are wave-uniform) and writes 64 consecutive rows of
// outputs[l].  The reference puts the level in blockIdx.y with 512-thread blocks (GC:908-909); the flat form needs no
// second grid dimension and launches 256-thread blocks.
//
// Forward: the 2^D corner rows of a (b, l) are gathered ONCE (a float2 per corner at F = 2) and serve both the
// interpolation and the reference's dy_dx formula, whose edge ends are exactly those corners.
//
// Backward (no float atomics; the fixed-point rule is written out in the header):
//   k_grid_gmax      max |grad| per level over the finite values (integer max of the bits, one atomic per workgroup)
//   k_grid_bwd       every contribution rounded once to int64 at the level's scale, added with 64-bit INTEGER atomics
//   k_grid_finalize  grad_embeddings = ldexp((float)sum, -s_l) over the whole table (0 outside the levels, NaN where a
//                    non-finite contribution landed)
//   k_grid_input_bwd grad_inputs, one thread per (b, d), l-then-ch order
//
// The row rule, the cell and the fixed-point scale are in grid_cell.h, shared with mix_grid.hip.
#include "common.h"
#include "grid_cell.h"
#include "../../include/bloomscene_grid.h"

namespace bsr {

// false: the point is outside [0, 1]^D (GC:133-138; NaN counts as outside)
template <int D>
__device__ __forceinline__ bool load_point(const float* __restrict__ inputs, long long b, float (&x)[D])
{
	bool in = true;
#pragma unroll
	for (int d = 0; d < D; d++) {
		x[d] = inputs[b * D + d];
		in = in && (x[d] >= 0.0f && x[d] <= 1.0f);
	}
	return in;
}

template <int D, int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_grid_fwd(int N, int L, int n_rows, const float* __restrict__ inputs,
                                                             const float* __restrict__ emb,
                                                             const int* __restrict__ offsets,
                                                             const int* __restrict__ resolutions,
                                                             float* __restrict__ outputs, float* __restrict__ dy_dx)
{
	const long long t = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (t >= (long long)N * L) return;
	const int l = (int)(t / N);
	const long long b = t - (long long)l * N;
	float x[D];
	const bool in = load_point<D>(inputs, b, x);
	Feat<F> out;
#pragma unroll
	for (int ch = 0; ch < F; ch++) out.v[ch] = 0.0f;
	float* dyp = dy_dx ? dy_dx + ((b * L + l) * D) * F : nullptr;
	if (!in) {
		store_feat<F>(outputs + t * F, out);
		if (dyp)
#pragma unroll
			for (int d = 0; d < D; d++) store_feat<F>(dyp + d * F, out);
		return;
	}
	const uint32_t off = (uint32_t)offsets[l];
	const uint32_t hs = (uint32_t)offsets[l + 1] - off;
	const uint32_t res = (uint32_t)resolutions[l];
	Cell<D> c;
	make_cell<D>(x, hs, res, (long long)n_rows - off, c);
	const float* g = emb + (size_t)off * F;
	Feat<F> val[1 << D];   // excluded corners read 0 (what the dy_dx formula wants, GC:639-642)
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (c.ok[k]) {
			val[k] = load_feat<F>(g + (size_t)c.row[k] * F);
		} else {
#pragma unroll
			for (int ch = 0; ch < F; ch++) val[k].v[ch] = 0.0f;
		}
	}
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (!c.ok[k]) continue;
		const float ww = c.w[k] * c.wn_re;
#pragma unroll
		for (int ch = 0; ch < F; ch++) out.v[ch] += ww * val[k].v[ch];   // GC:337-341
	}
	store_feat<F>(outputs + t * F, out);
	if (!dyp) return;
	// GC:588-660: for each dimension gd, 2^(D-1) edges along gd; edge idx fixes the other dimensions by its bits
	const float scale = (float)(res - 2u);
#pragma unroll
	for (int gd = 0; gd < D; gd++) {
		Feat<F> rg;
#pragma unroll
		for (int ch = 0; ch < F; ch++) rg.v[ch] = 0.0f;
#pragma unroll
		for (int idx = 0; idx < (1 << (D - 1)); idx++) {
			float w = scale;
			int corner = 0;
#pragma unroll
			for (int nd = 0; nd < D - 1; nd++) {
				const int d = nd >= gd ? nd + 1 : nd;
				if (((idx >> nd) & 1) == 0) {
					w *= 1.0f - c.pos[d];
				} else {
					w *= c.pos[d];
					corner |= 1 << d;
				}
			}
			const Feat<F>& lo = val[corner];
			const Feat<F>& hi = val[corner | (1 << gd)];
#pragma unroll
			for (int ch = 0; ch < F; ch++) rg.v[ch] += w * (hi.v[ch] - lo.v[ch]);   // (* pos_deriv = 1.0f: exact)
		}
		store_feat<F>(dyp + gd * F, rg);
	}
}

// ---- backward --------------------------------------------------------------------------------------------------------

// max |grad| of each level over its finite values: blockIdx.y = level, grid-stride over the level's N * F values
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_grid_gmax(long long per_level, const uint32_t* __restrict__ grad,
                                                              uint32_t* __restrict__ gmax)
{
	__shared__ uint32_t s_max[BSR_GRID_BLOCK / 64];
	const uint32_t* g = grad + (long long)blockIdx.y * per_level;
	uint32_t m = 0;
	for (long long i = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x; i < per_level;
	     i += (long long)gridDim.x * BSR_GRID_BLOCK) {
		const uint32_t a = g[i] & 0x7fffffffu;
		if (a < 0x7f800000u) m = max(m, a);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
	if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) {
#pragma unroll
		for (int w = 1; w < BSR_GRID_BLOCK / 64; w++) m = max(m, s_max[w]);
		if (m) atomicMax(gmax + blockIdx.y, m);
	}
}

template <int D, int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_grid_bwd(int N, int L, int n_rows, const float* __restrict__ grad,
                                                             const float* __restrict__ inputs,
                                                             const int* __restrict__ offsets,
                                                             const int* __restrict__ resolutions,
                                                             const uint32_t* __restrict__ gmax,
                                                             unsigned long long* __restrict__ acc,
                                                             uint32_t* __restrict__ nonfinite)
{
	const long long t = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (t >= (long long)N * L) return;
	const int l = (int)(t / N);
	const long long b = t - (long long)l * N;
	float x[D];
	if (!load_point<D>(inputs, b, x)) return;   // GC:713-718
	const uint32_t off = (uint32_t)offsets[l];
	const uint32_t hs = (uint32_t)offsets[l + 1] - off;
	const uint32_t res = (uint32_t)resolutions[l];
	const int s = grid_scale_exp(gmax[l], N, D);
	const Feat<F> g = load_feat<F>(grad + t * F);
	Cell<D> c;
	make_cell<D>(x, hs, res, (long long)n_rows - off, c);
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (!c.ok[k]) continue;
		const float ww = c.w[k] * c.wn_re;
		const size_t e0 = ((size_t)off + c.row[k]) * F;
#pragma unroll
		for (int ch = 0; ch < F; ch++)
			grid_contribute(ww * g.v[ch], s, e0 + ch, acc, nonfinite);   // GC:854: w_list[idx] * wn_re * grad_cur[c]
	}
}

// Every element of grad_embeddings: the level of its row (offsets in LDS), then the fixed-point sum scaled back
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_grid_finalize(long long n_elem, int F, int N, int D, int L,
                                                                  const int* __restrict__ offsets,
                                                                  const uint32_t* __restrict__ gmax,
                                                                  const long long* __restrict__ acc,
                                                                  const uint32_t* __restrict__ nonfinite,
                                                                  float* __restrict__ grad_embeddings)
{
	__shared__ int s_off[BSR_GRID_MAX_LEVELS + 1];
	__shared__ int s_exp[BSR_GRID_MAX_LEVELS];
	for (int i = threadIdx.x; i <= L; i += BSR_GRID_BLOCK) {
		s_off[i] = offsets[i];
		if (i < L) s_exp[i] = grid_scale_exp(gmax[i], N, D);
	}
	__syncthreads();
	const long long e = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (e >= n_elem) return;
	const long long row = e / F;
	int lvl = -1;
	for (int l = 0; l < L; l++)
		if (row >= s_off[l] && row < s_off[l + 1]) { lvl = l; break; }
	float r = 0.0f;
	if (lvl >= 0) {
		if ((nonfinite[e >> 5] >> (e & 31)) & 1u) r = __builtin_nanf("");
		else r = __builtin_ldexpf((float)acc[e], -s_exp[lvl]);
	}
	grad_embeddings[e] = r;
}

// GC:864-891
template <int D, int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_grid_input_bwd(int N, int L, const float* __restrict__ grad,
                                                                   const float* __restrict__ dy_dx,
                                                                   float* __restrict__ grad_inputs)
{
	const long long t = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (t >= (long long)N * D) return;
	const long long b = t / D;
	const int d = (int)(t - b * D);
	const float* dy = dy_dx + b * L * D * F + d * F;
	float r = 0.0f;
	for (int l = 0; l < L; l++) {
		const float* gl = grad + ((long long)l * N + b) * F;
#pragma unroll
		for (int ch = 0; ch < F; ch++) r += gl[ch] * dy[(long long)l * D * F + ch];
	}
	grad_inputs[t] = r;
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------

template <int D, int F>
static void launch_fwd(unsigned nb, hipStream_t st, int N, int L, int R, const float* in, const float* emb, const int* off,
                       const int* res, float* out, float* dy)
{
	hipLaunchKernelGGL((k_grid_fwd<D, F>), dim3(nb), dim3(BSR_GRID_BLOCK), 0, st, N, L, R, in, emb, off, res, out, dy);
}

template <int D, int F>
static void launch_bwd(unsigned nb, unsigned nb_in, hipStream_t st, int N, int L, int R, const float* grad, const float* in,
                       const int* off, const int* res, const uint32_t* gmax, unsigned long long* acc, uint32_t* nf,
                       const float* dy, float* gin)
{
	hipLaunchKernelGGL((k_grid_bwd<D, F>), dim3(nb), dim3(BSR_GRID_BLOCK), 0, st, N, L, R, grad, in, off, res, gmax, acc, nf);
	if (gin)
		hipLaunchKernelGGL((k_grid_input_bwd<D, F>), dim3(nb_in), dim3(BSR_GRID_BLOCK), 0, st, N, L, grad, dy, gin);
}

#define BSR_GRID_DISPATCH(D_, F_, CALL)                                                                      \
	switch ((D_) * 100 + (F_)) {                                                                              \
	case 101: CALL(1, 1); break; case 102: CALL(1, 2); break; case 104: CALL(1, 4); break; case 108: CALL(1, 8); break; \
	case 201: CALL(2, 1); break; case 202: CALL(2, 2); break; case 204: CALL(2, 4); break; case 208: CALL(2, 8); break; \
	case 301: CALL(3, 1); break; case 302: CALL(3, 2); break; case 304: CALL(3, 4); break; case 308: CALL(3, 8); break; \
	default: break;                                                                                           \
	}

static bool grid_shape_ok(const char* who, int N, int D, int F, int L)
{
	if (D < 1 || D > 3) return fail("%s: num_dim must be 1, 2 or 3 (got %d)", who, D), false;
	if (F != 1 && F != 2 && F != 4 && F != 8) return fail("%s: n_features must be 1, 2, 4 or 8 (got %d)", who, F), false;
	if (N < 0 || L < 0 || L > BSR_GRID_MAX_LEVELS)
		return fail("%s: need N >= 0 and 0 <= n_levels <= %d (got N=%d, n_levels=%d)", who, BSR_GRID_MAX_LEVELS, N, L), false;
	if ((long long)N * L >= (1ll << 31) || (long long)N * (D > F ? D : F) >= (1ll << 31))
		return fail("%s: N * n_levels must stay below 2^31", who), false;
	return true;
}

struct GridScratch {
	unsigned long long* acc;   // [n_rows * F] int64 sums
	uint32_t* nonfinite;       // [ceil(n_rows * F / 32)] bit per element
	uint32_t* gmax;            // [n_levels] max |grad| bits
	size_t bytes;
};

static GridScratch carve_grid_scratch(void* base, size_t n_rows, size_t F, size_t L)
{
	GridScratch s;
	const size_t n = n_rows * F;
	char* p = (char*)base;
	const size_t a = align_up(n * 8, 256), b = align_up((n + 31) / 32 * 4, 256), c = align_up(L * 4, 256);
	s.acc = (unsigned long long*)p;
	s.nonfinite = (uint32_t*)(p + a);
	s.gmax = (uint32_t*)(p + a + b);
	s.bytes = a + b + c;
	return s;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_grid_backward_scratch_bytes(int n_rows, int n_features, int n_levels)
{
	return carve_grid_scratch(nullptr, (size_t)(n_rows > 0 ? n_rows : 0), (size_t)(n_features > 0 ? n_features : 0),
	                          (size_t)(n_levels > 0 ? n_levels : 0)).bytes;
}

int bsr_grid_encode_forward(int N, int num_dim, int n_features, int n_levels, int n_rows, const float* inputs,
                            const float* embeddings, const int* offsets, const int* resolutions, float* outputs,
                            float* dy_dx, void* stream)
{
	const char* who = "bsr_grid_encode_forward";
	if (!grid_shape_ok(who, N, num_dim, n_features, n_levels)) return 1;
	if (n_rows < 0) return fail("%s: bad n_rows %d", who, n_rows);
	if (N == 0 || n_levels == 0) return 0;
	if (!inputs || !embeddings || !offsets || !resolutions || !outputs) return fail("%s: NULL buffer", who);
	const uintptr_t al = (uintptr_t)(n_features >= 4 ? 16 : 4 * n_features);
	if (((uintptr_t)embeddings | (uintptr_t)outputs | (uintptr_t)dy_dx) & (al - 1))
		return fail("%s: embeddings / outputs / dy_dx must be %d-byte aligned", who, (int)al);
	const unsigned nb = (unsigned)(((long long)N * n_levels + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK);
	hipStream_t st = (hipStream_t)stream;
#define BSR_CALL_FWD(D_, F_) launch_fwd<D_, F_>(nb, st, N, n_levels, n_rows, inputs, embeddings, offsets, resolutions, outputs, dy_dx)
	BSR_GRID_DISPATCH(num_dim, n_features, BSR_CALL_FWD)
#undef BSR_CALL_FWD
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_grid_encode_backward(int N, int num_dim, int n_features, int n_levels, int n_rows, const float* grad,
                             const float* inputs, const int* offsets, const int* resolutions, const float* dy_dx,
                             float* grad_embeddings, float* grad_inputs, void* scratch, void* stream)
{
	const char* who = "bsr_grid_encode_backward";
	if (!grid_shape_ok(who, N, num_dim, n_features, n_levels)) return 1;
	if (n_rows < 0 || (long long)n_rows * n_features >= (1ll << 38)) return fail("%s: bad n_rows %d", who, n_rows);
	const size_t n_elem = (size_t)n_rows * n_features;
	if (n_elem && !grad_embeddings) return fail("%s: grad_embeddings is NULL", who);
	hipStream_t st = (hipStream_t)stream;
	if (N == 0 || n_levels == 0) {
		if (n_elem && hipMemsetAsync(grad_embeddings, 0, n_elem * sizeof(float), st) != hipSuccess)
			return fail("%s: memset failed", who);
		return 0;
	}
	if (!grad || !inputs || !offsets || !resolutions || !scratch) return fail("%s: NULL buffer", who);
	if (grad_inputs && !dy_dx) return fail("%s: grad_inputs needs the forward's dy_dx", who);
	const uintptr_t al = (uintptr_t)(n_features >= 4 ? 16 : 4 * n_features);
	if ((uintptr_t)grad & (al - 1)) return fail("%s: grad must be %d-byte aligned", who, (int)al);
	if ((uintptr_t)scratch & 7) return fail("%s: scratch must be 8-byte aligned", who);
	const GridScratch s = carve_grid_scratch(scratch, (size_t)n_rows, (size_t)n_features, (size_t)n_levels);
	if (hipMemsetAsync(scratch, 0, s.bytes, st) != hipSuccess) return fail("%s: memset failed", who);
	const long long per_level = (long long)N * n_features;
	long long gb = (per_level + BSR_GRID_BLOCK * 8 - 1) / (BSR_GRID_BLOCK * 8);
	if (gb > 256) gb = 256;
	hipLaunchKernelGGL(k_grid_gmax, dim3((unsigned)gb, (unsigned)n_levels), dim3(BSR_GRID_BLOCK), 0, st, per_level,
	                   (const uint32_t*)grad, s.gmax);
	const unsigned nb = (unsigned)(((long long)N * n_levels + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK);
	const unsigned nb_in = (unsigned)(((long long)N * num_dim + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK);
#define BSR_CALL_BWD(D_, F_) launch_bwd<D_, F_>(nb, nb_in, st, N, n_levels, n_rows, grad, inputs, offsets, resolutions, s.gmax, \
                                                s.acc, s.nonfinite, dy_dx, grad_inputs)
	BSR_GRID_DISPATCH(num_dim, n_features, BSR_CALL_BWD)
#undef BSR_CALL_BWD
	if (n_elem) {
		hipLaunchKernelGGL(k_grid_finalize, dim3((unsigned)((n_elem + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK)),
		                   dim3(BSR_GRID_BLOCK), 0, st, (long long)n_elem, n_features, N, num_dim, n_levels, offsets,
		                   s.gmax, (const long long*)s.acc, s.nonfinite, grad_embeddings);
	}
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
