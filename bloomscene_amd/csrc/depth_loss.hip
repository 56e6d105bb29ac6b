// The depth-prior regularisation of BloomScene's loss for gfx950 (include/bloomscene_depth_loss.h): the min/max
// normalisations of bloomscene.py:298-305, HuberL1, CMD (a batch of one) and bilateral_filter of utils/loss.py, with
// the gradient to the rendered depth.
//
//   k_depth_extrema   min, max and their tie counts of D and P                          (only with `normalise`)
//   k_depth_maxdiff   M = max |r - o| and its tie count                                 (only with the value term)
//   k_depth_sums      the pixel sums of the three terms (optionally the maps) and out[4]
//   k_depth_grad      G = dloss / dr per pixel; without `normalise` the gradient itself, with it also sum G, sum G r
//   k_depth_grad_norm the gradient through the normalisation, with the extrema's shares  (only with `normalise`)
//
// TILING (k_depth_sums, k_depth_grad).  A workgroup of 256 threads owns a tile of 32 x 16 pixels (more tiles than
// BSR_DEPTH_MAX_BLOCKS: grid-stride), two pixels a thread (x = tid % 32, y = tid / 32 and y + 8).  It stages r of the tile
// and its halo of 2 pixels, 36 x 20, in LDS once -- coordinates clamped to the image, which is the replicate padding --
// and forms all 25 taps from LDS.  A 32-lane half reads 32 consecutive words of one row; the row stride is odd (37) so
// that the staging loop, whose halves straddle rows of 36, is conflict-free too.  rgb is read in place through its
// three strides.
// SUMS.  The header: per thread in fp64 in tile order, then grid_sum.h (which states the order) with one partial per
// sum per workgroup in the scratch; the extrema kernels use its ticket alone.  No float atomics; the only atomics are
// the integer tickets.
#include "common.h"
#include "grid_sum.h"
#include "../../include/bloomscene_depth_loss.h"

namespace bsr {

#define BSR_DEPTH_BLOCK 256
#define BSR_DEPTH_TW 32
#define BSR_DEPTH_TH 16
#define BSR_DEPTH_HALO 2
#define BSR_DEPTH_IN_W (BSR_DEPTH_TW + 2 * BSR_DEPTH_HALO)   // 36
#define BSR_DEPTH_IN_H (BSR_DEPTH_TH + 2 * BSR_DEPTH_HALO)   // 20
#define BSR_DEPTH_IN_STRIDE 37                               // staged rows (odd)
#define BSR_DEPTH_MAX_BLOCKS 16384   // tiled kernels; more tiles than this: grid-stride
#define BSR_DEPTH_LIN_BLOCKS 1024    // the two linear reductions, at most
#define BSR_DEPTH_LIN_PER_BLOCK 2048 // pixels a workgroup of a linear reduction takes before the grid grows no more
#define BSR_DEPTH_HEAD 256           // bytes of the scratch before the partials: four tickets, then sum G and sum G r
#define BSR_DEPTH_NSUM 5             // Sx, Sy, S, sum b, Q

static_assert(BSR_DEPTH_TW * BSR_DEPTH_TH == 2 * BSR_DEPTH_BLOCK, "two pixels a thread");

enum { TICKET_EXTREMA = 0, TICKET_MAXDIFF = 1, TICKET_SUMS = 2, TICKET_GRAD = 3 };
enum { SUM_X = 0, SUM_Y = 1, SUM_S = 2, SUM_B = 3, SUM_Q = 4 };

// the stats block (BSR_DEPTH_PRIOR_STATS_BYTES); every field is written by the forward kernel that owns it and read
// only by calls with the same terms and `normalise`
struct DepthStats {
	float minD, maxD, minP, maxP;
	float rgD, rgP, M, d;
	unsigned cnt_min, cnt_max, cnt_M, pad;
	double S, Q;
};
static_assert(sizeof(DepthStats) <= BSR_DEPTH_PRIOR_STATS_BYTES, "stats block");

struct Extrema {
	float lo, hi;
	unsigned n_lo, n_hi;
};
struct ExtremaPair {
	Extrema d, p;
};

struct DepthShape {
	int H, W;
	long long tiles_x, tiles_y, tiles;
	long long sy, sx, sc;   // of rgb, in elements
	int terms, normalise;
	float wv, wd, ws;
};

// scratch: [0, 16) four tickets; [64, 80) sum G, sum G r; from BSR_DEPTH_HEAD the linear reductions' partials
// (BSR_DEPTH_LIN_BLOCKS of 32 bytes), then BSR_DEPTH_NSUM fp64 per workgroup of a tiled kernel
struct DepthScratch {
	unsigned* ticket;
	double* gsum;
	void* lin;
	double* psum;
};

__host__ __device__ __forceinline__ constexpr float depth_sk(int di, int dj)
{
	const int k = di * di + dj * dj;
	return k == 0 ? BSR_DEPTH_PRIOR_SK0 : k == 1 ? BSR_DEPTH_PRIOR_SK1 : k == 2 ? BSR_DEPTH_PRIOR_SK2
	     : k == 4 ? BSR_DEPTH_PRIOR_SK4 : k == 5 ? BSR_DEPTH_PRIOR_SK5 : BSR_DEPTH_PRIOR_SK8;
}

static unsigned depth_tile_blocks(long long tiles)
{
	return (unsigned)(tiles < 1 ? 1 : (tiles < BSR_DEPTH_MAX_BLOCKS ? tiles : BSR_DEPTH_MAX_BLOCKS));
}
static unsigned depth_lin_blocks(long long n)
{
	const long long b = (n + BSR_DEPTH_LIN_PER_BLOCK - 1) / BSR_DEPTH_LIN_PER_BLOCK;
	return (unsigned)(b < 1 ? 1 : (b < BSR_DEPTH_LIN_BLOCKS ? b : BSR_DEPTH_LIN_BLOCKS));
}

__device__ __forceinline__ float depth_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float depth_clamp(float x) { return x < -1e6f ? -1e6f : (x > 1e6f ? 1e6f : x); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// r or o of one depth
__device__ __forceinline__ float depth_norm(float v, float lo, float rg, int normalise) { return normalise ? (v - lo) / rg : v; }

// (lo, n_lo) and (hi, n_hi) of two sets: exact whatever the order
__device__ __forceinline__ void extrema_add(Extrema& a, float lo, unsigned n_lo, float hi, unsigned n_hi)
{
	if (n_lo && (a.n_lo == 0 || lo < a.lo)) { a.lo = lo; a.n_lo = n_lo; }
	else if (n_lo && lo == a.lo) a.n_lo += n_lo;
	if (n_hi && (a.n_hi == 0 || hi > a.hi)) { a.hi = hi; a.n_hi = n_hi; }
	else if (n_hi && hi == a.hi) a.n_hi += n_hi;
}

// all threads' extrema -> thread 0 of the workgroup
__device__ __forceinline__ void extrema_block(Extrema& a)
{
	__shared__ Extrema s_e[BSR_DEPTH_BLOCK / 64];
	const int tid = threadIdx.x;
	for (int o = 32; o > 0; o >>= 1) {
		const float lo = __shfl_xor(a.lo, o), hi = __shfl_xor(a.hi, o);
		const unsigned n_lo = __shfl_xor(a.n_lo, o), n_hi = __shfl_xor(a.n_hi, o);
		extrema_add(a, lo, n_lo, hi, n_hi);
	}
	__syncthreads();   // (s_e of an earlier call)
	if ((tid & 63) == 0) s_e[tid >> 6] = a;
	__syncthreads();
	if (tid == 0)
		for (int w = 1; w < BSR_DEPTH_BLOCK / 64; w++) extrema_add(a, s_e[w].lo, s_e[w].n_lo, s_e[w].hi, s_e[w].n_hi);
}

__device__ __forceinline__ Extrema extrema_none()
{
	Extrema e;
	e.lo = 0.0f;
	e.hi = 0.0f;
	e.n_lo = 0;
	e.n_hi = 0;
	return e;
}

__global__ void __launch_bounds__(BSR_DEPTH_BLOCK) k_depth_extrema(long long n, const float* __restrict__ D,
                                                                   const float* __restrict__ P, DepthStats* stats,
                                                                   DepthScratch sc)
{
	const int tid = threadIdx.x;
	ExtremaPair* part = (ExtremaPair*)sc.lin;
	Extrema d = extrema_none(), p = extrema_none();
	for (long long i = (long long)blockIdx.x * BSR_DEPTH_BLOCK + tid; i < n; i += (long long)gridDim.x * BSR_DEPTH_BLOCK) {
		const float dv = D[i], pv = P[i];
		extrema_add(d, dv, 1u, dv, 1u);
		extrema_add(p, pv, 1u, pv, 1u);
	}
	extrema_block(d);
	extrema_block(p);
	if (tid == 0) {
		part[blockIdx.x].d = d;
		part[blockIdx.x].p = p;
	}
	if (!grid_last_ticket(&sc.ticket[TICKET_EXTREMA])) return;
	d = extrema_none();
	p = extrema_none();
	for (unsigned b = tid; b < gridDim.x; b += BSR_DEPTH_BLOCK) {
		const unsigned* w = (const unsigned*)&part[b];
		extrema_add(d, __uint_as_float(load_u32(w + 0)), load_u32(w + 2), __uint_as_float(load_u32(w + 1)), load_u32(w + 3));
		extrema_add(p, __uint_as_float(load_u32(w + 4)), load_u32(w + 6), __uint_as_float(load_u32(w + 5)), load_u32(w + 7));
	}
	extrema_block(d);
	extrema_block(p);
	if (tid == 0) {
		stats->minD = d.lo;
		stats->maxD = d.hi;
		stats->minP = p.lo;
		stats->maxP = p.hi;
		stats->rgD = (d.hi - d.lo) + 1e-8f;
		stats->rgP = (p.hi - p.lo) + 1e-8f;
		stats->cnt_min = d.n_lo;
		stats->cnt_max = d.n_hi;
	}
}

__global__ void __launch_bounds__(BSR_DEPTH_BLOCK) k_depth_maxdiff(long long n, int normalise, const float* __restrict__ D,
                                                                   const float* __restrict__ P, DepthStats* stats,
                                                                   DepthScratch sc)
{
	const int tid = threadIdx.x;
	Extrema* part = (Extrema*)sc.lin;
	float minD = 0.0f, rgD = 1.0f, minP = 0.0f, rgP = 1.0f;
	if (normalise) {
		minD = stats->minD;
		rgD = stats->rgD;
		minP = stats->minP;
		rgP = stats->rgP;
	}
	Extrema m = extrema_none();
	for (long long i = (long long)blockIdx.x * BSR_DEPTH_BLOCK + tid; i < n; i += (long long)gridDim.x * BSR_DEPTH_BLOCK) {
		const float l1 = fabsf(depth_norm(D[i], minD, rgD, normalise) - depth_norm(P[i], minP, rgP, normalise));
		extrema_add(m, 0.0f, 0u, l1, 1u);
	}
	extrema_block(m);
	if (tid == 0) part[blockIdx.x] = m;
	if (!grid_last_ticket(&sc.ticket[TICKET_MAXDIFF])) return;
	m = extrema_none();
	for (unsigned b = tid; b < gridDim.x; b += BSR_DEPTH_BLOCK) {
		const unsigned* w = (const unsigned*)&part[b];
		extrema_add(m, 0.0f, 0u, __uint_as_float(load_u32(w + 1)), load_u32(w + 3));
	}
	extrema_block(m);
	if (tid == 0) {
		stats->M = m.hi;
		stats->d = BSR_DEPTH_PRIOR_TRESH * m.hi;
		stats->cnt_M = m.n_hi;
	}
}

struct DepthTile {
	int x0, y0;
};
__device__ __forceinline__ DepthTile depth_tile(const DepthShape& s, long long tile)
{
	DepthTile t;
	t.y0 = (int)(tile / s.tiles_x) * BSR_DEPTH_TH;
	t.x0 = (int)(tile % s.tiles_x) * BSR_DEPTH_TW;
	return t;
}

// r of the tile with its halo -> dst, coordinates clamped to the image
__device__ __forceinline__ void stage_r(const DepthShape& s, const DepthTile& t, const float* __restrict__ D, float minD, float rgD,
                                        float* dst)
{
	for (int i = threadIdx.x; i < BSR_DEPTH_IN_H * BSR_DEPTH_IN_W; i += BSR_DEPTH_BLOCK) {
		const int r = i / BSR_DEPTH_IN_W, cx = i - r * BSR_DEPTH_IN_W;
		const int gy = clampi(t.y0 - BSR_DEPTH_HALO + r, s.H - 1), gx = clampi(t.x0 - BSR_DEPTH_HALO + cx, s.W - 1);
		dst[r * BSR_DEPTH_IN_STRIDE + cx] = depth_norm(D[(long long)gy * s.W + gx], minD, rgD, s.normalise);
	}
}

// ex and ey of the header at (gx, gy)
__device__ __forceinline__ void edge_weights(const DepthShape& s, const float* __restrict__ rgb, int gx, int gy, float& ex, float& ey)
{
	const float* at = rgb + (long long)gy * s.sy + (long long)gx * s.sx;
	const float c0 = at[0], c1 = at[s.sc], c2 = at[2 * s.sc];
	ex = 0.0f;
	ey = 0.0f;
	if (gx < s.W - 1) {
		const float* n = at + s.sx;
		const float gr = ((fabsf(c0 - n[0]) + fabsf(c1 - n[s.sc])) + fabsf(c2 - n[2 * s.sc])) / 3.0f;
		ex = bsr_expf(-gr);
	}
	if (gy < s.H - 1) {
		const float* n = at + s.sy;
		const float gr = ((fabsf(c0 - n[0]) + fabsf(c1 - n[s.sc])) + fabsf(c2 - n[2 * s.sc])) / 3.0f;
		ey = bsr_expf(-gr);
	}
}

// t'(x) of the header
__device__ __forceinline__ float bilateral_slope(float x)
{
	return bsr_expf(-(fabsf(x) / BSR_DEPTH_PRIOR_COLOR_DIV)) * (2.0f * x - depth_sign(x) * ((x * x) / BSR_DEPTH_PRIOR_COLOR_DIV));
}

__global__ void __launch_bounds__(BSR_DEPTH_BLOCK) k_depth_sums(DepthShape s, const float* __restrict__ D,
                                                                const float* __restrict__ P, const float* __restrict__ rgb,
                                                                double K, float* __restrict__ maps, float* __restrict__ out,
                                                                DepthStats* stats, DepthScratch sc)
{
	__shared__ float s_r[BSR_DEPTH_IN_H * BSR_DEPTH_IN_STRIDE];
	const int tid = threadIdx.x;
	const long long HW = (long long)s.H * s.W;
	const bool value = s.terms & BSR_DEPTH_PRIOR_VALUE, domin = s.terms & BSR_DEPTH_PRIOR_DOMIN, smooth = s.terms & BSR_DEPTH_PRIOR_SMOOTH;
	float minD = 0.0f, rgD = 1.0f, minP = 0.0f, rgP = 1.0f, d = 0.0f;
	if (s.normalise) {
		minD = stats->minD;
		rgD = stats->rgD;
		minP = stats->minP;
		rgP = stats->rgP;
	}
	if (value) d = stats->d;
	const float nx = (float)((long long)s.H * (s.W - 1)), ny = (float)((long long)(s.H - 1) * s.W);
	double sums[BSR_DEPTH_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
	for (long long tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		const DepthTile t = depth_tile(s, tile);
		stage_r(s, t, D, minD, rgD, s_r);
		__syncthreads();
		const int x = tid & (BSR_DEPTH_TW - 1);
		for (int j = 0; j < 2; j++) {
			const int y = (tid >> 5) + j * (BSR_DEPTH_TH / 2);
			const int gx = t.x0 + x, gy = t.y0 + y;
			if (gx >= s.W || gy >= s.H) continue;
			const long long at = (long long)gy * s.W + gx;
			const float* centre = &s_r[(y + BSR_DEPTH_HALO) * BSR_DEPTH_IN_STRIDE + x + BSR_DEPTH_HALO];
			const float r = centre[0];
			const float o = depth_norm(P[at], minP, rgP, s.normalise);
			float h = 0.0f, b = 0.0f;
			if (value) {
				const float e = r - o, l1 = fabsf(e);
				const bool linear = l1 >= d;
				h = linear ? l1 : (e * e + d * d) / (2.0f * d);
				float ex, ey;
				edge_weights(s, rgb, gx, gy, ex, ey);
				if (gx < s.W - 1) sums[SUM_X] += (double)(ex * h);
				if (gy < s.H - 1) sums[SUM_Y] += (double)(ey * h);
				if (!linear) {
					const float a = ex / nx + ey / ny;
					sums[SUM_Q] += (double)(a * (0.5f - (e * e) / (2.0f * (d * d))));
				}
			}
			if (domin) {
				const float ec = depth_clamp(r) - depth_clamp(o);
				const float tt = fabsf(ec) + 1e-6f;
				float pw = tt * tt;
				pw = pw > 1e6f ? 1e6f : pw;
				sums[SUM_S] += (double)pw;
			}
			if (smooth) {
#pragma unroll
				for (int i = -2; i <= 2; i++)
#pragma unroll
					for (int jj = -2; jj <= 2; jj++) {
						const float delta = r - centre[i * BSR_DEPTH_IN_STRIDE + jj];
						b = b + (depth_sk(i, jj) * bsr_expf(-(fabsf(delta) / BSR_DEPTH_PRIOR_COLOR_DIV))) * (delta * delta);
					}
				sums[SUM_B] += (double)b;
			}
			if (maps) {
				maps[BSR_DEPTH_PRIOR_MAP_R * HW + at] = r;
				maps[BSR_DEPTH_PRIOR_MAP_H * HW + at] = h;
				maps[BSR_DEPTH_PRIOR_MAP_B * HW + at] = b;
			}
		}
		__syncthreads();   // (the next tile's staging overwrites what this pass read)
	}
	if (grid_sum<BSR_DEPTH_NSUM, BSR_DEPTH_BLOCK>(sums, &sc.ticket[TICKET_SUMS], sc.psum)) {
		double Lv = 0.0, Ld = 0.0, Ls = 0.0, loss = 0.0;
		if (value) {
			Lv = sums[SUM_X] / (double)((long long)s.H * (s.W - 1)) + sums[SUM_Y] / (double)((long long)(s.H - 1) * s.W);
			loss = (double)s.wv * Lv;
		}
		if (domin) {
			const double S = sums[SUM_S];
			Ld = sqrt((S > 1e6 ? 1e6 : S) + 1e-6) + K;
			loss = loss + (double)s.wd * Ld;
		}
		if (smooth) {
			Ls = sums[SUM_B] / (double)HW;
			loss = loss + (double)s.ws * Ls;
		}
		out[0] = (float)loss;
		out[1] = (float)Lv;
		out[2] = (float)Ld;
		out[3] = (float)Ls;
		stats->S = sums[SUM_S];
		stats->Q = sums[SUM_Q];
	}
}

__global__ void __launch_bounds__(BSR_DEPTH_BLOCK) k_depth_grad(DepthShape s, const float* __restrict__ D,
                                                                const float* __restrict__ P, const float* __restrict__ rgb,
                                                                const DepthStats* __restrict__ stats, const float* __restrict__ g,
                                                                float* __restrict__ grad, DepthScratch sc)
{
	__shared__ float s_r[BSR_DEPTH_IN_H * BSR_DEPTH_IN_STRIDE];
	const int tid = threadIdx.x;
	const long long HW = (long long)s.H * s.W;
	const bool value = s.terms & BSR_DEPTH_PRIOR_VALUE, domin = s.terms & BSR_DEPTH_PRIOR_DOMIN, smooth = s.terms & BSR_DEPTH_PRIOR_SMOOTH;
	float minD = 0.0f, rgD = 1.0f, minP = 0.0f, rgP = 1.0f, d = 0.0f, M = 0.0f, qM = 0.0f, sd = 1.0f;
	bool sum_open = false;
	if (s.normalise) {
		minD = stats->minD;
		rgD = stats->rgD;
		minP = stats->minP;
		rgP = stats->rgP;
	}
	if (value) {
		d = stats->d;
		M = stats->M;
		qM = (float)((double)BSR_DEPTH_PRIOR_TRESH * stats->Q / (double)stats->cnt_M);
	}
	if (domin) {
		const double S = stats->S;
		sum_open = S <= 1e6;
		sd = (float)sqrt((S > 1e6 ? 1e6 : S) + 1e-6);
	}
	const float nx = (float)((long long)s.H * (s.W - 1)), ny = (float)((long long)(s.H - 1) * s.W);
	const float gv = g[0];
	double sums[2] = {0.0, 0.0};
	for (long long tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		const DepthTile t = depth_tile(s, tile);
		stage_r(s, t, D, minD, rgD, s_r);
		__syncthreads();
		const int x = tid & (BSR_DEPTH_TW - 1);
		for (int j = 0; j < 2; j++) {
			const int y = (tid >> 5) + j * (BSR_DEPTH_TH / 2);
			const int gx = t.x0 + x, gy = t.y0 + y;
			if (gx >= s.W || gy >= s.H) continue;
			const long long at = (long long)gy * s.W + gx;
			const float* centre = &s_r[(y + BSR_DEPTH_HALO) * BSR_DEPTH_IN_STRIDE + x + BSR_DEPTH_HALO];
			const float r = centre[0];
			const float o = depth_norm(P[at], minP, rgP, s.normalise);
			float G = 0.0f;
			if (value) {
				const float e = r - o, l1 = fabsf(e), sg = depth_sign(e);
				float ex, ey;
				edge_weights(s, rgb, gx, gy, ex, ey);
				const float a = ex / nx + ey / ny;
				float Gv = l1 >= d ? a * sg : a * (e / d);
				if (l1 == M) Gv = Gv + sg * qM;
				G = s.wv * Gv;
			}
			if (domin) {
				const float ec = depth_clamp(r) - depth_clamp(o);
				const float tt = fabsf(ec) + 1e-6f;
				const bool open = sum_open && fabsf(r) <= 1e6f && tt * tt <= 1e6f;
				const float Gd = open ? depth_sign(ec) * (tt / sd) : 0.0f;
				G = value ? G + s.wd * Gd : s.wd * Gd;
			}
			if (smooth) {
				float a1 = 0.0f, a2 = 0.0f;
#pragma unroll
				for (int i = -2; i <= 2; i++)
#pragma unroll
					for (int jj = -2; jj <= 2; jj++) a1 = a1 + depth_sk(i, jj) * bilateral_slope(r - centre[i * BSR_DEPTH_IN_STRIDE + jj]);
				// the taps (i, jj) of p = q + (pa, pb) that replicate padding maps onto q: one, -(pa, pb), unless q is
				// on the border, where every tap reaching past it lands on q too.  Two pixels or more from every border
				// the loop below is a1's with every term negated (t' is odd, sk symmetric): the same bits
				const bool inner = gy >= 2 && gy < s.H - 2 && gx >= 2 && gx < s.W - 2;
				if (inner) a2 = -a1;
				for (int pa = -2; pa <= 2 && !inner; pa++) {
					const int py = gy + pa;
					if (py < 0 || py >= s.H) continue;
					const int i_lo = gy == 0 ? -2 : -pa, i_hi = gy == s.H - 1 ? 2 : -pa;
					for (int pb = -2; pb <= 2; pb++) {
						const int px = gx + pb;
						if (px < 0 || px >= s.W) continue;
						const int j_lo = gx == 0 ? -2 : -pb, j_hi = gx == s.W - 1 ? 2 : -pb;
						const float slope = bilateral_slope(centre[pa * BSR_DEPTH_IN_STRIDE + pb] - r);
						for (int i = i_lo; i <= i_hi; i++)
							for (int jj = j_lo; jj <= j_hi; jj++) a2 = a2 + depth_sk(i, jj) * slope;
					}
				}
				const float Gs = (a1 - a2) / (float)HW;
				G = (value || domin) ? G + s.ws * Gs : s.ws * Gs;
			}
			if (s.normalise) {
				grad[at] = G;
				sums[0] += (double)G;
				sums[1] += (double)G * (double)r;
			} else {
				grad[at] = gv * G;
			}
		}
		__syncthreads();
	}
	if (!s.normalise) return;   // (uniform over the grid)
	if (grid_sum<2, BSR_DEPTH_BLOCK>(sums, &sc.ticket[TICKET_GRAD], sc.psum)) {
		sc.gsum[0] = sums[0];
		sc.gsum[1] = sums[1];
	}
}

__global__ void __launch_bounds__(BSR_DEPTH_BLOCK) k_depth_grad_norm(long long n, const float* __restrict__ D,
                                                                     const DepthStats* __restrict__ stats,
                                                                     const double* __restrict__ gsum,
                                                                     const float* __restrict__ g, float* __restrict__ grad)
{
	const float minD = stats->minD, maxD = stats->maxD, rgD = stats->rgD, gv = g[0];
	const double sG = gsum[0], sGr = gsum[1];
	const float qmin = (float)((sGr - sG) / (double)rgD / (double)stats->cnt_min);
	const float qmax = (float)(-sGr / (double)rgD / (double)stats->cnt_max);
	for (long long i = (long long)blockIdx.x * BSR_DEPTH_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BSR_DEPTH_BLOCK) {
		const float dv = D[i];
		grad[i] = gv * ((grad[i] / rgD + (dv == minD ? qmin : 0.0f)) + (dv == maxD ? qmax : 0.0f));
	}
}

// the checks both entry points share; fills the shape
static int depth_shape(const char* who, int H, int W, long long sy, long long sx, long long sc, int terms, float wv, float wd,
                       float ws, int normalise, DepthShape& s)
{
	if (H < 1 || W < 1) return fail("%s: need H, W >= 1 (got %d, %d)", who, H, W);
	if ((long long)H * W >= (1LL << 31)) return fail("%s: H * W must be below 2^31 (got %d * %d)", who, H, W);
	if (terms & ~(BSR_DEPTH_PRIOR_VALUE | BSR_DEPTH_PRIOR_DOMIN | BSR_DEPTH_PRIOR_SMOOTH)) return fail("%s: unknown bits in terms (%d)", who, terms);
	if ((terms & BSR_DEPTH_PRIOR_VALUE) && (H < 2 || W < 2)) return fail("%s: the value term needs H, W >= 2 (got %d, %d)", who, H, W);
	s.H = H;
	s.W = W;
	s.tiles_x = ((long long)W + BSR_DEPTH_TW - 1) / BSR_DEPTH_TW;
	s.tiles_y = ((long long)H + BSR_DEPTH_TH - 1) / BSR_DEPTH_TH;
	s.tiles = s.tiles_x * s.tiles_y;
	s.sy = sy;
	s.sx = sx;
	s.sc = sc;
	s.terms = terms;
	s.normalise = normalise != 0;
	s.wv = wv;
	s.wd = wd;
	s.ws = ws;
	return 0;
}

static long long depth_tiles(int H, int W)
{
	return (((long long)W + BSR_DEPTH_TW - 1) / BSR_DEPTH_TW) * (((long long)H + BSR_DEPTH_TH - 1) / BSR_DEPTH_TH);
}

static DepthScratch depth_scratch(void* scratch)
{
	DepthScratch sc;
	sc.ticket = (unsigned*)scratch;
	sc.gsum = (double*)((char*)scratch + 64);
	sc.lin = (char*)scratch + BSR_DEPTH_HEAD;
	sc.psum = (double*)((char*)scratch + BSR_DEPTH_HEAD + (size_t)BSR_DEPTH_LIN_BLOCKS * sizeof(ExtremaPair));
	return sc;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_depth_prior_scratch_bytes(int H, int W)
{
	if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return 0;
	return align_up(BSR_DEPTH_HEAD + (size_t)BSR_DEPTH_LIN_BLOCKS * sizeof(ExtremaPair) +
	                (size_t)depth_tile_blocks(depth_tiles(H, W)) * BSR_DEPTH_NSUM * sizeof(double), 256);
}

int bsr_depth_prior_forward(int H, int W, const float* D, const float* P, const float* rgb, long long sy, long long sx,
                            long long sc_, int terms, float wv, float wd, float ws, int normalise, float* maps, float* out,
                            void* stats, void* scratch, void* stream)
{
	const char* who = "bsr_depth_prior_forward";
	DepthShape s;
	if (depth_shape(who, H, W, sy, sx, sc_, terms, wv, wd, ws, normalise, s)) return 1;
	if (!D || !P || !out || !stats || !scratch) return fail("%s: NULL operand", who);
	if ((terms & BSR_DEPTH_PRIOR_VALUE) && !rgb) return fail("%s: the value term needs rgb", who);
	if (((uintptr_t)D | (uintptr_t)P | (uintptr_t)rgb | (uintptr_t)maps | (uintptr_t)out) & 3)
		return fail("%s: operands and outputs must be 4-byte aligned", who);
	if ((uintptr_t)stats & 7) return fail("%s: stats must be 8-byte aligned", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const long long n = (long long)H * W;
	const DepthScratch sc = depth_scratch(scratch);
	if (hipMemsetAsync(sc.ticket, 0, 16, st) != hipSuccess) return fail("%s: memset failed", who);
	if (s.normalise) hipLaunchKernelGGL(k_depth_extrema, dim3(depth_lin_blocks(n)), dim3(BSR_DEPTH_BLOCK), 0, st, n, D, P, (DepthStats*)stats, sc);
	if (terms & BSR_DEPTH_PRIOR_VALUE)
		hipLaunchKernelGGL(k_depth_maxdiff, dim3(depth_lin_blocks(n)), dim3(BSR_DEPTH_BLOCK), 0, st, n, s.normalise, D, P, (DepthStats*)stats, sc);
	const double tiny = (double)1e-6f;
	const double K = 4.0 * sqrt((double)n * (tiny * tiny) + 1e-6);
	hipLaunchKernelGGL(k_depth_sums, dim3(depth_tile_blocks(s.tiles)), dim3(BSR_DEPTH_BLOCK), 0, st, s, D, P, rgb, K, maps, out,
	                   (DepthStats*)stats, sc);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_depth_prior_backward(int H, int W, const float* D, const float* P, const float* rgb, long long sy, long long sx,
                             long long sc_, int terms, float wv, float wd, float ws, int normalise, const void* stats,
                             const float* g, float* grad, void* scratch, void* stream)
{
	const char* who = "bsr_depth_prior_backward";
	DepthShape s;
	if (depth_shape(who, H, W, sy, sx, sc_, terms, wv, wd, ws, normalise, s)) return 1;
	if (!D || !P || !stats || !g || !grad || !scratch) return fail("%s: NULL operand", who);
	if ((terms & BSR_DEPTH_PRIOR_VALUE) && !rgb) return fail("%s: the value term needs rgb", who);
	if (((uintptr_t)D | (uintptr_t)P | (uintptr_t)rgb | (uintptr_t)g | (uintptr_t)grad) & 3)
		return fail("%s: operands and the gradient must be 4-byte aligned", who);
	if ((uintptr_t)stats & 7) return fail("%s: stats must be 8-byte aligned", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const long long n = (long long)H * W;
	const DepthScratch sc = depth_scratch(scratch);
	if (s.normalise && hipMemsetAsync(sc.ticket, 0, 16, st) != hipSuccess) return fail("%s: memset failed", who);
	hipLaunchKernelGGL(k_depth_grad, dim3(depth_tile_blocks(s.tiles)), dim3(BSR_DEPTH_BLOCK), 0, st, s, D, P, rgb,
	                   (const DepthStats*)stats, g, grad, sc);
	if (s.normalise)
		hipLaunchKernelGGL(k_depth_grad_norm, dim3(depth_lin_blocks(n)), dim3(BSR_DEPTH_BLOCK), 0, st, n, D, (const DepthStats*)stats,
		                   (const double*)sc.gsum, g, grad);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
