// The fused mixed 3D/2D binary hash-grid encoding for gfx950 (include/bloomscene_mix_grid.h): BloomScene's
// calc_interp_feat -- the normalisation, up to four GridEncoders on coordinate selections of one point, STE_binary read
// as a sign at the corner, and the concatenated [n, C] output -- forward and backward, every launch over all grids.
//
// Forward, ONE launch (k_mix_fwd): a 256-thread workgroup owns 64 consecutive points across all levels of all grids.
// A lane is a point (its normalised coordinates are computed once), a wave walks the (grid, level) slots wave, wave + 4, ...
// so that D, the table, the offset, the resolution and the dense-or-hashed choice stay wave-uniform (the property
// grid.hip's launch shape builds on).  The F values of a (point, slot) go into an LDS tile [64 points][w columns] at an
// ODD pitch (w | 1: lanes of a wave write a column conflict-free); after a barrier the workgroup stores the tile row by
// row with consecutive lanes on consecutive floats -- at w == C the 64 rows are one contiguous run of 64 C floats -- so no
// lane ever writes 4F bytes at a stride of 4C.  w = min(C, 128) columns per round, C / w rounds: at most 33 KiB of
// dynamic LDS, 12.5 KiB at the shipped C = 48.  dy_dx, written only when asked for, goes out per lane like grid.hip's.
//
// Backward (no float atomics; the fixed-point rule of include/bloomscene_grid.h per (grid, level)):
//   k_mix_zero       the one zero fill of the caller's scratch for all grids.  A kernel and not hipMemsetAsync: replayed from a
//                    captured graph, a memset node in front of tables this small left the sums of the previous replay
//                    in place on the MI355X (docs/EXPERIMENTS.md), a kernel node does what it does outside a graph
//   k_mix_gmax       max |grad_out| per slot over the finite values, one coalesced sweep of [n, C], maxima in LDS
//   k_mix_bwd        the forward's shape with the grad_out tile loaded through LDS; int64 atomics into each table's sums
//   k_mix_finalize   every element of every trainable table: ldexp((float)sum, -s), NaN where a non-finite contribution
//                    landed, and STE_binary's gate (|p| <= 1) in the same store
//   k_mix_input_bwd  grad_x, one thread per (point, coordinate)
// Frozen tables (grad_params[g] == NULL) have no slots in k_mix_bwd, no elements in k_mix_finalize and no scratch.
#include "common.h"
#include "grid_cell.h"
#include "../../include/bloomscene_mix_grid.h"

namespace bsr {

#define BSR_MIX_POINTS 64       // points of a workgroup = lanes of a wave
#define BSR_MIX_WAVES (BSR_GRID_BLOCK / 64)
#define BSR_MIX_TILE_COLS 128   // columns of one round (a multiple of every supported F)

// Everything the kernels need to know about the grids, passed by value
struct MixDesc {
	int G, total_levels;
	int C;                                   // F * sum L_g: columns of out / grad_out
	int W;                                   // F * sum L_g D_g: columns of dy_dx
	int n_levels[BSR_MIX_MAX_GRIDS];
	int slot0[BSR_MIX_MAX_GRIDS + 1];        // first (grid, level) slot of each grid
	int dy0[BSR_MIX_MAX_GRIDS];              // first dy_dx column of each grid
	int n_dims[BSR_MIX_MAX_GRIDS];
	int dims[BSR_MIX_MAX_GRIDS][3];
	int n_rows[BSR_MIX_MAX_GRIDS];
	const float* params[BSR_MIX_MAX_GRIDS];
	const int* offsets[BSR_MIX_MAX_GRIDS];
	const int* resolutions[BSR_MIX_MAX_GRIDS];
	// backward only (all NULL for a frozen grid)
	float* grad_params[BSR_MIX_MAX_GRIDS];
	unsigned long long* acc[BSR_MIX_MAX_GRIDS];
	uint32_t* nonfinite[BSR_MIX_MAX_GRIDS];
	long long elem0[BSR_MIX_MAX_GRIDS + 1];  // first element of each grid in k_mix_finalize's flat index
};

// a / b correctly rounded: the double quotient of two fp32 values rounds to fp32 without a double-rounding error (53 >= 2 * 24 + 2)
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// STE_binary.forward at one value (utils/encodings.py:181-184): +1 for p >= 0 (-0 included), -1 for p < 0, 0 for NaN
__device__ __forceinline__ float ste_sign(float p) { return p >= 0.0f ? 1.0f : (p < 0.0f ? -1.0f : 0.0f); }

// u = (x - min) / (max - min) (scene/gaussian_model.py:417), or x itself without bounds
__device__ __forceinline__ void mix_load_point(const float* __restrict__ x, long long xs, long long b,
                                               const float* __restrict__ bmin, const float* __restrict__ bmax, float (&u)[3])
{
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const float v = x[b * xs + d];
		u[d] = bmin ? div_rn(v - bmin[d], bmax[d] - bmin[d]) : v;
	}
}

__device__ __forceinline__ int mix_grid_of_slot(const MixDesc& m, int s)
{
	int g = 0;
	while (g + 1 < m.G && s >= m.slot0[g + 1]) g++;
	return g;
}

// The coordinates grid g selects; false: outside [0, 1]^D on them (GC:133-138; NaN counts as outside)
template <int D>
__device__ __forceinline__ bool mix_select(const MixDesc& m, int g, const float (&u)[3], float (&xg)[D])
{
	bool in = true;
#pragma unroll
	for (int d = 0; d < D; d++) {
		const int k = m.dims[g][d];
		xg[d] = k == 0 ? u[0] : (k == 1 ? u[1] : u[2]);
		in = in && (xg[d] >= 0.0f && xg[d] <= 1.0f);
	}
	return in;
}

// One (point, grid, level): exactly k_grid_fwd's body on u[dims_g], the corner value read through the sign
template <int D, int F>
__device__ __forceinline__ Feat<F> mix_encode_one(const MixDesc& m, int g, int l, const float (&u)[3], int binary, float* dyp)
{
	Feat<F> out;
#pragma unroll
	for (int ch = 0; ch < F; ch++) out.v[ch] = 0.0f;
	float xg[D];
	if (!mix_select<D>(m, g, u, xg)) {
		if (dyp)
#pragma unroll
			for (int d = 0; d < D; d++) store_feat<F>(dyp + d * F, out);
		return out;
	}
	const uint32_t off = (uint32_t)m.offsets[g][l];
	const uint32_t hs = (uint32_t)m.offsets[g][l + 1] - off;
	const uint32_t res = (uint32_t)m.resolutions[g][l];
	Cell<D> c;
	make_cell<D>(xg, hs, res, (long long)m.n_rows[g] - off, c);
	const float* tab = m.params[g] + (size_t)off * F;
	Feat<F> val[1 << D];
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (c.ok[k]) {
			val[k] = load_feat<F>(tab + (size_t)c.row[k] * F);
			if (binary)
#pragma unroll
				for (int ch = 0; ch < F; ch++) val[k].v[ch] = ste_sign(val[k].v[ch]);
		} else {
#pragma unroll
			for (int ch = 0; ch < F; ch++) val[k].v[ch] = 0.0f;
		}
	}
	out = interpolate<D, F>(c, val);
	if (dyp) store_dy_dx<D, F>(c, res, val, dyp);
	return out;
}

template <int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_fwd(const MixDesc m, int n, int binary, const float* __restrict__ x,
                                                            long long xs, const float* __restrict__ bmin,
                                                            const float* __restrict__ bmax, float* __restrict__ out,
                                                            float* __restrict__ dy_dx)
{
	extern __shared__ float tile[];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const long long b0 = (long long)blockIdx.x * BSR_MIX_POINTS;
	const long long b = b0 + lane;
	const bool live = b < n;
	float u[3] = {-1.0f, -1.0f, -1.0f};   // (a lane beyond n is "outside": zeros into tile rows nobody stores)
	if (live) mix_load_point(x, xs, b, bmin, bmax, u);
	const int w = m.C < BSR_MIX_TILE_COLS ? m.C : BSR_MIX_TILE_COLS;
	const int pitch = w | 1;
	const int rows = n - b0 < BSR_MIX_POINTS ? (int)(n - b0) : BSR_MIX_POINTS;
	for (int c0 = 0; c0 < m.C; c0 += w) {
		const int c1 = c0 + w < m.C ? c0 + w : m.C;
		for (int s = c0 / F + wave; s < c1 / F; s += BSR_MIX_WAVES) {
			const int g = mix_grid_of_slot(m, s);
			const int l = s - m.slot0[g];
			const int D = m.n_dims[g];
			float* dyp = (dy_dx && live) ? dy_dx + b * m.W + m.dy0[g] + (long long)l * D * F : nullptr;
			Feat<F> o;
			if (D == 3) o = mix_encode_one<3, F>(m, g, l, u, binary, dyp);
			else if (D == 2) o = mix_encode_one<2, F>(m, g, l, u, binary, dyp);
			else o = mix_encode_one<1, F>(m, g, l, u, binary, dyp);
			float* t = tile + lane * pitch + (s * F - c0);
#pragma unroll
			for (int ch = 0; ch < F; ch++) t[ch] = o.v[ch];
		}
		__syncthreads();
		const int wc = c1 - c0;
		for (int i = threadIdx.x; i < rows * wc; i += BSR_GRID_BLOCK) {
			const int p = i / wc, c = i - p * wc;
			out[(b0 + p) * m.C + c0 + c] = tile[p * pitch + c];
		}
		__syncthreads();
	}
}

// ---- backward --------------------------------------------------------------------------------------------------------

// The one zero fill of the scratch (sums, non-finite bits and maxima of all grids): a kernel, so that a captured backward
// consists of kernel nodes only
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_zero(unsigned long long* __restrict__ p, long long n)
{
	for (long long i = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BSR_GRID_BLOCK)
		p[i] = 0ull;
}

// max |grad_out| of each slot over its finite values: one sweep of [n, C] rows, per-slot maxima in LDS, then one global
// integer atomic per slot and workgroup
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_gmax(int n, int C, int log2F, const uint32_t* __restrict__ grad,
                                                             long long gs, uint32_t* __restrict__ gmax)
{
	__shared__ uint32_t s_max[BSR_GRID_MAX_LEVELS];
	if (threadIdx.x < BSR_GRID_MAX_LEVELS) s_max[threadIdx.x] = 0u;
	__syncthreads();
	const long long total = (long long)n * C;
	for (long long i = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x; i < total;
	     i += (long long)gridDim.x * BSR_GRID_BLOCK) {
		const long long b = i / C;
		const int c = (int)(i - b * C);
		const uint32_t a = grad[b * gs + c] & 0x7fffffffu;
		if (a < 0x7f800000u) {
			const int s = c >> log2F;
			if (a > ((volatile uint32_t*)s_max)[s]) atomicMax(&s_max[s], a);   // (the plain read only skips adds that cannot win)
		}
	}
	__syncthreads();
	if (threadIdx.x < (C >> log2F) && s_max[threadIdx.x]) atomicMax(gmax + threadIdx.x, s_max[threadIdx.x]);
}

template <int D, int F>
__device__ __forceinline__ void mix_contribute_one(const MixDesc& m, int g, int l, int n, const float (&u)[3],
                                                   const Feat<F>& go, uint32_t gbits)
{
	float xg[D];
	if (!mix_select<D>(m, g, u, xg)) return;   // GC:713-718
	const uint32_t off = (uint32_t)m.offsets[g][l];
	const uint32_t hs = (uint32_t)m.offsets[g][l + 1] - off;
	const uint32_t res = (uint32_t)m.resolutions[g][l];
	const int s = grid_scale_exp(gbits, n, D);
	Cell<D> c;
	make_cell<D>(xg, hs, res, (long long)m.n_rows[g] - off, c);
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (!c.ok[k]) continue;
		const float ww = c.w[k] * c.wn_re;
		const size_t e0 = ((size_t)off + c.row[k]) * F;
#pragma unroll
		for (int ch = 0; ch < F; ch++)
			grid_contribute(ww * go.v[ch], s, e0 + ch, m.acc[g], m.nonfinite[g]);   // GC:854
	}
}

template <int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_bwd(const MixDesc m, int n, const float* __restrict__ grad, long long gs,
                                                            const float* __restrict__ x, long long xs,
                                                            const float* __restrict__ bmin, const float* __restrict__ bmax,
                                                            const uint32_t* __restrict__ gmax)
{
	extern __shared__ float tile[];
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const long long b0 = (long long)blockIdx.x * BSR_MIX_POINTS;
	const long long b = b0 + lane;
	const bool live = b < n;
	float u[3] = {-1.0f, -1.0f, -1.0f};
	if (live) mix_load_point(x, xs, b, bmin, bmax, u);
	const int w = m.C < BSR_MIX_TILE_COLS ? m.C : BSR_MIX_TILE_COLS;
	const int pitch = w | 1;
	const int rows = n - b0 < BSR_MIX_POINTS ? (int)(n - b0) : BSR_MIX_POINTS;
	for (int c0 = 0; c0 < m.C; c0 += w) {
		const int c1 = c0 + w < m.C ? c0 + w : m.C;
		const int wc = c1 - c0;
		for (int i = threadIdx.x; i < rows * wc; i += BSR_GRID_BLOCK) {
			const int p = i / wc, c = i - p * wc;
			tile[p * pitch + c] = grad[(b0 + p) * gs + c0 + c];
		}
		__syncthreads();
		for (int s = c0 / F + wave; s < c1 / F; s += BSR_MIX_WAVES) {
			const int g = mix_grid_of_slot(m, s);
			if (!m.acc[g] || !live) continue;   // a frozen table; a lane beyond n (its tile row was not loaded)
			const int l = s - m.slot0[g];
			const int D = m.n_dims[g];
			Feat<F> go;
			const float* t = tile + lane * pitch + (s * F - c0);
#pragma unroll
			for (int ch = 0; ch < F; ch++) go.v[ch] = t[ch];
			const uint32_t gbits = gmax[s];
			if (D == 3) mix_contribute_one<3, F>(m, g, l, n, u, go, gbits);
			else if (D == 2) mix_contribute_one<2, F>(m, g, l, n, u, go, gbits);
			else mix_contribute_one<1, F>(m, g, l, n, u, go, gbits);
		}
		__syncthreads();
	}
}

// Every element of every trainable table: its grid from elem0, the level of its row (offsets in LDS), the fixed-point sum
// scaled back, and STE_binary's gate (utils/encodings.py:187-192: clamp(p, -1, 1) == p, false for NaN) in the same store
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_finalize(const MixDesc m, int n, int F, int binary,
                                                                 const uint32_t* __restrict__ gmax)
{
	__shared__ int s_off[BSR_GRID_MAX_LEVELS + BSR_MIX_MAX_GRIDS];   // grid g's L_g + 1 offsets from slot0[g] + g on
	__shared__ int s_exp[BSR_GRID_MAX_LEVELS];
	for (int g = 0; g < m.G; g++) {
		for (int i = threadIdx.x; i <= m.n_levels[g]; i += BSR_GRID_BLOCK) {
			s_off[m.slot0[g] + g + i] = m.offsets[g][i];
			if (i < m.n_levels[g]) s_exp[m.slot0[g] + i] = grid_scale_exp(gmax[m.slot0[g] + i], n, m.n_dims[g]);
		}
	}
	__syncthreads();
	const long long e = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (e >= m.elem0[m.G]) return;
	int g = 0;
	while (g + 1 < m.G && e >= m.elem0[g + 1]) g++;
	const long long le = e - m.elem0[g];
	const long long row = le / F;
	const int* off = s_off + m.slot0[g] + g;
	int lvl = -1;
	for (int l = 0; l < m.n_levels[g]; l++)
		if (row >= off[l] && row < off[l + 1]) { lvl = l; break; }
	float r = 0.0f;
	if (lvl >= 0) {
		if ((m.nonfinite[g][le >> 5] >> (le & 31)) & 1u) r = __builtin_nanf("");
		else r = __builtin_ldexpf((float)((const long long*)m.acc[g])[le], -s_exp[m.slot0[g] + lvl]);
	}
	if (binary && !(__builtin_fabsf(m.params[g][le]) <= 1.0f)) r = 0.0f;
	m.grad_params[g][le] = r;
}

// grad_x: r_g[d] in the l-then-ch order of GC:864-891, summed over the grids that select d in ascending g, then the
// normalisation's factor
template <int F>
__global__ void __launch_bounds__(BSR_GRID_BLOCK) k_mix_input_bwd(const MixDesc m, int n, const float* __restrict__ grad,
                                                                  long long gs, const float* __restrict__ dy_dx,
                                                                  const float* __restrict__ bmin,
                                                                  const float* __restrict__ bmax, float* __restrict__ grad_x)
{
	const long long t = (long long)blockIdx.x * BSR_GRID_BLOCK + threadIdx.x;
	if (t >= (long long)n * 3) return;
	const long long b = t / 3;
	const int d = (int)(t - b * 3);
	float sum = 0.0f;
	bool first = true;
	for (int g = 0; g < m.G; g++) {
		const int D = m.n_dims[g];
		int k = -1;
		for (int j = 0; j < D; j++)
			if (m.dims[g][j] == d) k = j;
		if (k < 0) continue;
		const float* dy = dy_dx + b * m.W + m.dy0[g] + k * F;
		const float* gl = grad + b * gs + (long long)m.slot0[g] * F;
		float r = 0.0f;
		for (int l = 0; l < m.n_levels[g]; l++) {
#pragma unroll
			for (int ch = 0; ch < F; ch++) r += gl[l * F + ch] * dy[(long long)l * D * F + ch];
		}
		sum = first ? r : sum + r;
		first = false;
	}
	if (bmin) sum = div_rn(sum, bmax[d] - bmin[d]);
	grad_x[t] = sum;
}

// ---- host ------------------------------------------------------------------------------------------------------------

struct MixScratch {
	unsigned long long* acc[BSR_MIX_MAX_GRIDS];
	uint32_t* nonfinite[BSR_MIX_MAX_GRIDS];
	uint32_t* gmax;
	size_t bytes;
};

// rows[g] == 0: grid g is frozen and takes no room
static MixScratch carve_mix_scratch(void* base, int G, const int* rows, size_t F, size_t total_levels)
{
	MixScratch s;
	char* p = (char*)base;
	size_t at = 0;
	for (int g = 0; g < BSR_MIX_MAX_GRIDS; g++) {
		const size_t n = g < G && rows && rows[g] > 0 ? (size_t)rows[g] * F : 0;
		s.acc[g] = n ? (unsigned long long*)(p + at) : nullptr;
		at += align_up(n * 8, 256);
		s.nonfinite[g] = n ? (uint32_t*)(p + at) : nullptr;
		at += align_up((n + 31) / 32 * 4, 256);
	}
	s.gmax = (uint32_t*)(p + at);
	at += align_up(total_levels * 4, 256);
	s.bytes = at;
	return s;
}

// The shape checks of both entry points and the descriptor; 0 on success
static int mix_describe(const char* who, int N, int G, int F, const float* const* params, const int* const* offsets,
                        const int* const* resolutions, const int* n_levels, const int* n_rows, const int* n_dims,
                        const int* dims, MixDesc& m)
{
	if (G < 1 || G > BSR_MIX_MAX_GRIDS) return fail("%s: n_grids must be in [1, %d] (got %d)", who, BSR_MIX_MAX_GRIDS, G);
	if (F != 1 && F != 2 && F != 4 && F != 8) return fail("%s: n_features must be 1, 2, 4 or 8 (got %d)", who, F);
	if (N < 0) return fail("%s: need N >= 0 (got %d)", who, N);
	if (!params || !offsets || !resolutions || !n_levels || !n_rows || !n_dims || !dims) return fail("%s: NULL grid array", who);
	m = MixDesc{};
	m.G = G;
	int slots = 0, dy = 0;
	const uintptr_t al = (uintptr_t)(F >= 4 ? 16 : 4 * F);
	for (int g = 0; g < G; g++) {
		if (n_levels[g] < 0 || n_levels[g] > BSR_GRID_MAX_LEVELS) return fail("%s: grid %d: bad n_levels %d", who, g, n_levels[g]);
		if (n_rows[g] < 0 || (long long)n_rows[g] * F >= (1ll << 38)) return fail("%s: grid %d: bad n_rows %d", who, g, n_rows[g]);
		if (n_dims[g] < 1 || n_dims[g] > 3) return fail("%s: grid %d: 1 to 3 coordinates (got %d)", who, g, n_dims[g]);
		for (int k = 0; k < n_dims[g]; k++) {
			const int d = dims[g * 3 + k];
			if (d < 0 || d > 2 || (k > 0 && d <= dims[g * 3 + k - 1]))
				return fail("%s: grid %d: dims must be distinct ascending indices into (x, y, z)", who, g);
			m.dims[g][k] = d;
		}
		if (n_levels[g] > 0 && (!params[g] || !offsets[g] || !resolutions[g])) return fail("%s: grid %d: NULL buffer", who, g);
		if ((uintptr_t)params[g] & (al - 1)) return fail("%s: grid %d: params must be %d-byte aligned", who, g, (int)al);
		m.n_levels[g] = n_levels[g];
		m.slot0[g] = slots;
		m.dy0[g] = dy;
		m.n_dims[g] = n_dims[g];
		m.n_rows[g] = n_rows[g];
		m.params[g] = params[g];
		m.offsets[g] = offsets[g];
		m.resolutions[g] = resolutions[g];
		slots += n_levels[g];
		dy += n_levels[g] * n_dims[g] * F;
	}
	for (int g = G; g <= BSR_MIX_MAX_GRIDS; g++) m.slot0[g] = slots;
	if (slots > BSR_GRID_MAX_LEVELS) return fail("%s: at most %d levels over all grids (got %d)", who, BSR_GRID_MAX_LEVELS, slots);
	m.total_levels = slots;
	m.C = slots * F;
	m.W = dy;
	if ((long long)N * m.C >= (1ll << 31)) return fail("%s: N * n_features * (levels of all grids) must stay below 2^31", who);
	return 0;
}

static size_t mix_tile_bytes(const MixDesc& m)
{
	const int w = m.C < BSR_MIX_TILE_COLS ? m.C : BSR_MIX_TILE_COLS;
	return (size_t)BSR_MIX_POINTS * (size_t)(w | 1) * sizeof(float);
}

#define BSR_MIX_DISPATCH(F_, CALL) \
	switch (F_) { case 1: CALL(1); break; case 2: CALL(2); break; case 4: CALL(4); break; case 8: CALL(8); break; default: break; }

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_mix_grid_backward_scratch_bytes(int n_grids, const int* n_rows, int n_features, int total_levels)
{
	if (n_grids < 0 || n_grids > BSR_MIX_MAX_GRIDS) n_grids = 0;
	return carve_mix_scratch(nullptr, n_grids, n_rows, (size_t)(n_features > 0 ? n_features : 0),
	                         (size_t)(total_levels > 0 ? total_levels : 0)).bytes;
}

int bsr_mix_grid_forward(int N, int n_grids, int n_features, int binary, const float* x, long long x_stride,
                         const float* bound_min, const float* bound_max, const float* const* params,
                         const int* const* offsets, const int* const* resolutions, const int* n_levels, const int* n_rows,
                         const int* n_dims, const int* dims, float* out, float* dy_dx, void* stream)
{
	const char* who = "bsr_mix_grid_forward";
	MixDesc m;
	if (mix_describe(who, N, n_grids, n_features, params, offsets, resolutions, n_levels, n_rows, n_dims, dims, m)) return 1;
	if (N == 0 || m.total_levels == 0) return 0;
	if (!x || !out) return fail("%s: NULL buffer", who);
	if (x_stride < 3) return fail("%s: x_stride must be at least 3 (got %lld)", who, x_stride);
	if ((bound_min == nullptr) != (bound_max == nullptr)) return fail("%s: bound_min and bound_max come together", who);
	const uintptr_t al = (uintptr_t)(n_features >= 4 ? 16 : 4 * n_features);
	if ((uintptr_t)dy_dx & (al - 1)) return fail("%s: dy_dx must be %d-byte aligned", who, (int)al);
	const unsigned nb = (unsigned)(((long long)N + BSR_MIX_POINTS - 1) / BSR_MIX_POINTS);
	const size_t lds = mix_tile_bytes(m);
	hipStream_t st = (hipStream_t)stream;
#define BSR_CALL(F_) hipLaunchKernelGGL((k_mix_fwd<F_>), dim3(nb), dim3(BSR_GRID_BLOCK), lds, st, m, N, binary, x, x_stride, \
                                        bound_min, bound_max, out, dy_dx)
	BSR_MIX_DISPATCH(n_features, BSR_CALL)
#undef BSR_CALL
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_mix_grid_backward(int N, int n_grids, int n_features, int binary, const float* grad_out, long long grad_stride,
                          const float* x, long long x_stride, const float* bound_min, const float* bound_max,
                          const float* const* params, const int* const* offsets, const int* const* resolutions,
                          const int* n_levels, const int* n_rows, const int* n_dims, const int* dims, const float* dy_dx,
                          float* const* grad_params, float* grad_x, void* scratch, void* stream)
{
	const char* who = "bsr_mix_grid_backward";
	MixDesc m;
	if (mix_describe(who, N, n_grids, n_features, params, offsets, resolutions, n_levels, n_rows, n_dims, dims, m)) return 1;
	if (!grad_params) return fail("%s: NULL grid array", who);
	hipStream_t st = (hipStream_t)stream;
	int rows[BSR_MIX_MAX_GRIDS] = {0, 0, 0, 0};
	bool trainable = false;
	for (int g = 0; g < n_grids; g++) {
		rows[g] = grad_params[g] ? n_rows[g] : 0;
		trainable = trainable || rows[g] > 0;
	}
	if (N == 0 || m.total_levels == 0) {
		for (int g = 0; g < n_grids; g++)
			if (rows[g] > 0 && hipMemsetAsync(grad_params[g], 0, (size_t)rows[g] * n_features * sizeof(float), st) != hipSuccess)
				return fail("%s: memset failed", who);
		return 0;
	}
	if (!grad_out || !x) return fail("%s: NULL buffer", who);
	if (x_stride < 3 || grad_stride < m.C) return fail("%s: x_stride must be at least 3 and grad_stride at least C", who);
	if ((bound_min == nullptr) != (bound_max == nullptr)) return fail("%s: bound_min and bound_max come together", who);
	if (grad_x && !dy_dx) return fail("%s: grad_x needs the forward's dy_dx", who);
	if (trainable) {
		if (!scratch || ((uintptr_t)scratch & 7)) return fail("%s: scratch must be given, 8-byte aligned", who);
		const MixScratch s = carve_mix_scratch(scratch, n_grids, rows, (size_t)n_features, (size_t)m.total_levels);
		const long long words = (long long)(s.bytes / 8);
		long long zb = (words + BSR_GRID_BLOCK * 4 - 1) / (BSR_GRID_BLOCK * 4);
		if (zb > 2048) zb = 2048;
		hipLaunchKernelGGL(k_mix_zero, dim3((unsigned)zb), dim3(BSR_GRID_BLOCK), 0, st, (unsigned long long*)scratch, words);
		long long at = 0;
		for (int g = 0; g < n_grids; g++) {
			m.elem0[g] = at;
			if (rows[g] > 0) {
				m.grad_params[g] = grad_params[g];
				m.acc[g] = s.acc[g];
				m.nonfinite[g] = s.nonfinite[g];
				at += (long long)rows[g] * n_features;
			}
		}
		for (int g = n_grids; g <= BSR_MIX_MAX_GRIDS; g++) m.elem0[g] = at;
		int log2F = 0;
		while ((1 << log2F) < n_features) log2F++;
		long long gb = ((long long)N * m.C + BSR_GRID_BLOCK * 8 - 1) / (BSR_GRID_BLOCK * 8);
		if (gb > 1024) gb = 1024;
		hipLaunchKernelGGL(k_mix_gmax, dim3((unsigned)gb), dim3(BSR_GRID_BLOCK), 0, st, N, m.C, log2F, (const uint32_t*)grad_out,
		                   grad_stride, s.gmax);
		const unsigned nb = (unsigned)(((long long)N + BSR_MIX_POINTS - 1) / BSR_MIX_POINTS);
		const size_t lds = mix_tile_bytes(m);
#define BSR_CALL(F_) hipLaunchKernelGGL((k_mix_bwd<F_>), dim3(nb), dim3(BSR_GRID_BLOCK), lds, st, m, N, grad_out, grad_stride, x, \
                                        x_stride, bound_min, bound_max, (const uint32_t*)s.gmax)
		BSR_MIX_DISPATCH(n_features, BSR_CALL)
#undef BSR_CALL
		hipLaunchKernelGGL(k_mix_finalize, dim3((unsigned)((at + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK)), dim3(BSR_GRID_BLOCK), 0, st,
		                   m, N, n_features, binary, (const uint32_t*)s.gmax);
	}
	if (grad_x) {
		const unsigned nb_in = (unsigned)(((long long)N * 3 + BSR_GRID_BLOCK - 1) / BSR_GRID_BLOCK);
#define BSR_CALL(F_) hipLaunchKernelGGL((k_mix_input_bwd<F_>), dim3(nb_in), dim3(BSR_GRID_BLOCK), 0, st, m, N, grad_out, grad_stride, \
                                        dy_dx, bound_min, bound_max, grad_x)
		BSR_MIX_DISPATCH(n_features, BSR_CALL)
#undef BSR_CALL
	}
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
