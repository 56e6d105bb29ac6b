// The photometric term of BloomScene's loss for gfx950 (include/bloomscene_loss.h): l1_loss and ssim of
// utils/loss.py:83-134 and their combination of bloomscene.py:284-287, with the gradient to the first image.
//
//   k_photometric_fwd   the SSIM map's three partial derivatives per pixel (optionally the map), and {loss, L1, S}
//   k_photometric_bwd   the gradient: the partials convolved once more, combined with the sign of the difference
//
// TILING.  A workgroup of 256 threads owns a tile of 32 x 16 pixels of one (b, c) plane (more tiles than
// BSR_LOSS_MAX_BLOCKS: grid-stride).  It stages the tile and its halo of 5 pixels, 42 x 26, of every input plane in LDS
// -- zeros outside the image, which is the padding -- runs the row pass over the 26 x 32 positions the column pass needs and
// leaves its results in LDS, then the column pass with two pixels a thread (x = tid % 32, y = tid / 32 and y + 8).  Every
// (input, tap) product is formed from LDS: global memory is read once per staged element.
// LDS BANKS.  ds_read_b32 conflicts count per 32-lane half.  A half always holds 32 consecutive x of ONE row (both passes
// are indexed row * 32 + x), so every access is to 32 consecutive words whatever the row stride; the strides are odd (43
// and 33) all the same, so that the staging loop, whose halves straddle rows of 42, stays conflict-free too.
// SUMS.  bloomscene_loss.h: per thread in fp64 in tile order, then grid_sum.h (which states the order) with two partials
// per workgroup in the scratch.  No float atomics; the only atomic is the integer ticket.
// COST.  About 380 fp32 operations and 93 LDS reads a pixel forward, 185 and 87 backward.  At [3, 512, 512] that is 1536
// tiles, one round of resident workgroups (26 KB of LDS: six a CU), and 0.09 ms for both kernels (docs/EXPERIMENTS.md).
#include "common.h"
#include "grid_sum.h"
#include "../../include/bloomscene_loss.h"

namespace bsr {

#define BSR_LOSS_BLOCK 256
#define BSR_LOSS_TW 32
#define BSR_LOSS_TH 16
#define BSR_LOSS_HALO 5
#define BSR_LOSS_IN_W (BSR_LOSS_TW + 2 * BSR_LOSS_HALO)   // 42
#define BSR_LOSS_IN_H (BSR_LOSS_TH + 2 * BSR_LOSS_HALO)   // 26
#define BSR_LOSS_IN_STRIDE 43                             // staged rows (odd)
#define BSR_LOSS_ROW_STRIDE 33                            // row-pass rows (odd)
#define BSR_LOSS_IN_WORDS (BSR_LOSS_IN_H * BSR_LOSS_IN_STRIDE)
#define BSR_LOSS_ROW_WORDS (BSR_LOSS_IN_H * BSR_LOSS_ROW_STRIDE)
#define BSR_LOSS_MAX_BLOCKS 16384   // more tiles than this: grid-stride
#define BSR_LOSS_HEAD 256           // bytes of the scratch before the partials (the ticket)

static_assert(BSR_LOSS_TW * BSR_LOSS_TH == 2 * BSR_LOSS_BLOCK, "two pixels a thread");

struct LossShape {
	int H, W;
	long long planes;             // B * C
	long long tiles_x, tiles_y;   // per plane
	long long tiles;
};

// scratch: [0, 4) the ticket; from BSR_LOSS_HEAD two fp64 per workgroup (|img - gt|, then m)
struct LossScratch {
	unsigned* ticket;
	double* psum;
};

__host__ __device__ __forceinline__ constexpr float loss_window(int k)
{
	const int j = k < 6 ? k : 10 - k;
	return j == 0 ? BSR_PHOTOMETRIC_W0 : j == 1 ? BSR_PHOTOMETRIC_W1 : j == 2 ? BSR_PHOTOMETRIC_W2
	     : j == 3 ? BSR_PHOTOMETRIC_W3 : j == 4 ? BSR_PHOTOMETRIC_W4 : BSR_PHOTOMETRIC_W5;
}

static unsigned loss_blocks(long long tiles)
{
	return (unsigned)(tiles < 1 ? 1 : (tiles < BSR_LOSS_MAX_BLOCKS ? tiles : BSR_LOSS_MAX_BLOCKS));
}

struct LossTile {
	long long base;   // of the plane, in elements
	int x0, y0;
};
__device__ __forceinline__ LossTile loss_tile(const LossShape& s, long long tile)
{
	const long long per = s.tiles_x * s.tiles_y;
	const long long plane = tile / per, in = tile - plane * per;
	LossTile t;
	t.base = plane * (long long)s.H * (long long)s.W;
	t.y0 = (int)(in / s.tiles_x) * BSR_LOSS_TH;
	t.x0 = (int)(in % s.tiles_x) * BSR_LOSS_TW;
	return t;
}

// the tile of `plane` with its halo -> dst, zeros outside the image
__device__ __forceinline__ void stage_tile(const LossShape& s, const LossTile& t, const float* __restrict__ plane, float* dst)
{
	for (int i = threadIdx.x; i < BSR_LOSS_IN_H * BSR_LOSS_IN_W; i += BSR_LOSS_BLOCK) {
		const int r = i / BSR_LOSS_IN_W, cx = i - r * BSR_LOSS_IN_W;
		const int gy = t.y0 - BSR_LOSS_HALO + r, gx = t.x0 - BSR_LOSS_HALO + cx;
		const bool in = gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
		dst[r * BSR_LOSS_IN_STRIDE + cx] = in ? plane[t.base + (long long)gy * s.W + gx] : 0.0f;
	}
}

// the column pass at (x, y) of the tile over one row-pass plane
__device__ __forceinline__ float column_pass(const float* rows, int x, int y)
{
	float acc = 0.0f;
#pragma unroll
	for (int k = 0; k < 11; k++) acc = acc + loss_window(k) * rows[(y + k) * BSR_LOSS_ROW_STRIDE + x];
	return acc;
}

__global__ void __launch_bounds__(BSR_LOSS_BLOCK) k_photometric_fwd(LossShape s, const float* __restrict__ img,
                                                                    const float* __restrict__ gt, float lambda,
                                                                    float* __restrict__ partials, float* __restrict__ ssim_map,
                                                                    float* __restrict__ out, LossScratch sc)
{
	__shared__ float s_in[2][BSR_LOSS_IN_WORDS];     // img, gt
	__shared__ float s_row[5][BSR_LOSS_ROW_WORDS];   // the row pass of img, gt, img img, gt gt, img gt
	const int tid = threadIdx.x;
	const long long N = s.planes * (long long)s.H * (long long)s.W;
	double sums[2] = {0.0, 0.0};   // |img - gt|, m
	for (long long tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		const LossTile t = loss_tile(s, tile);
		stage_tile(s, t, img, s_in[0]);
		stage_tile(s, t, gt, s_in[1]);
		__syncthreads();
		for (int i = tid; i < BSR_LOSS_IN_H * BSR_LOSS_TW; i += BSR_LOSS_BLOCK) {
			const int r = i / BSR_LOSS_TW, x = i - r * BSR_LOSS_TW;
			const float* pi = &s_in[0][r * BSR_LOSS_IN_STRIDE + x];
			const float* pg = &s_in[1][r * BSR_LOSS_IN_STRIDE + x];
			float h1 = 0.0f, h2 = 0.0f, h11 = 0.0f, h22 = 0.0f, h12 = 0.0f;
#pragma unroll
			for (int k = 0; k < 11; k++) {
				const float w = loss_window(k), a = pi[k], b = pg[k];
				h1 = h1 + w * a;
				h2 = h2 + w * b;
				h11 = h11 + w * (a * a);
				h22 = h22 + w * (b * b);
				h12 = h12 + w * (a * b);
			}
			const int o = r * BSR_LOSS_ROW_STRIDE + x;
			s_row[0][o] = h1;
			s_row[1][o] = h2;
			s_row[2][o] = h11;
			s_row[3][o] = h22;
			s_row[4][o] = h12;
		}
		__syncthreads();
		const int x = tid & (BSR_LOSS_TW - 1);
		for (int j = 0; j < 2; j++) {
			const int y = (tid >> 5) + j * (BSR_LOSS_TH / 2);
			const int gx = t.x0 + x, gy = t.y0 + y;
			if (gx >= s.W || gy >= s.H) continue;
			const float mu1 = column_pass(s_row[0], x, y), mu2 = column_pass(s_row[1], x, y);
			const float e11 = column_pass(s_row[2], x, y), e22 = column_pass(s_row[3], x, y), e12 = column_pass(s_row[4], x, y);
			const float p12 = mu1 * mu2, q1 = mu1 * mu1, q2 = mu2 * mu2;
			const float s1 = e11 - q1, s2 = e22 - q2, s12 = e12 - p12;
			const float a = 2.0f * p12 + BSR_PHOTOMETRIC_C1, b = 2.0f * s12 + BSR_PHOTOMETRIC_C2;
			const float c = (q1 + q2) + BSR_PHOTOMETRIC_C1, d = (s1 + s2) + BSR_PHOTOMETRIC_C2;
			const float ab = a * b, cd = c * d;
			const float m = ab / cd;
			const long long at = t.base + (long long)gy * s.W + gx;
			if (partials) {
				const float p_mu = ((2.0f * mu2) * (b - a)) / cd - (((2.0f * mu1) * ab) * (d - c)) / (cd * cd);
				const float p_e11 = -(ab / (cd * d));
				const float p_e12 = (2.0f * a) / cd;
				partials[BSR_PHOTOMETRIC_P_MU * N + at] = p_mu;
				partials[BSR_PHOTOMETRIC_P_E11 * N + at] = p_e11;
				partials[BSR_PHOTOMETRIC_P_E12 * N + at] = p_e12;
			}
			if (ssim_map) ssim_map[at] = m;
			const int centre = (y + BSR_LOSS_HALO) * BSR_LOSS_IN_STRIDE + x + BSR_LOSS_HALO;
			sums[0] += (double)fabsf(s_in[0][centre] - s_in[1][centre]);
			sums[1] += (double)m;
		}
		__syncthreads();   // (the next tile's staging overwrites what this pass read)
	}
	if (grid_sum<2, BSR_LOSS_BLOCK>(sums, sc.ticket, sc.psum)) {
		const double n = (double)N, lam = (double)lambda;
		const double l1 = sums[0] / n, ssim = sums[1] / n;
		const double first = (1.0 - lam) * l1, second = lam * (1.0 - ssim);
		out[0] = (float)(first + second);
		out[1] = (float)l1;
		out[2] = (float)ssim;
	}
}

__global__ void __launch_bounds__(BSR_LOSS_BLOCK) k_photometric_bwd(LossShape s, const float* __restrict__ img,
                                                                    const float* __restrict__ gt,
                                                                    const float* __restrict__ partials, float kl, float ks,
                                                                    const float* __restrict__ g, float* __restrict__ grad)
{
	__shared__ float s_in[3][BSR_LOSS_IN_WORDS];     // pMu, pE11, pE12
	__shared__ float s_row[3][BSR_LOSS_ROW_WORDS];
	const int tid = threadIdx.x;
	const long long N = s.planes * (long long)s.H * (long long)s.W;
	const float gv = g[0];
	for (long long tile = blockIdx.x; tile < s.tiles; tile += gridDim.x) {
		const LossTile t = loss_tile(s, tile);
		for (int p = 0; p < 3; p++) stage_tile(s, t, partials + p * N, s_in[p]);
		__syncthreads();
		for (int i = tid; i < BSR_LOSS_IN_H * BSR_LOSS_TW; i += BSR_LOSS_BLOCK) {
			const int r = i / BSR_LOSS_TW, x = i - r * BSR_LOSS_TW;
			const int from = r * BSR_LOSS_IN_STRIDE + x, o = r * BSR_LOSS_ROW_STRIDE + x;
			float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
#pragma unroll
			for (int k = 0; k < 11; k++) {
				const float w = loss_window(k);
				h0 = h0 + w * s_in[0][from + k];
				h1 = h1 + w * s_in[1][from + k];
				h2 = h2 + w * s_in[2][from + k];
			}
			s_row[0][o] = h0;
			s_row[1][o] = h1;
			s_row[2][o] = h2;
		}
		__syncthreads();
		const int x = tid & (BSR_LOSS_TW - 1);
		for (int j = 0; j < 2; j++) {
			const int y = (tid >> 5) + j * (BSR_LOSS_TH / 2);
			const int gx = t.x0 + x, gy = t.y0 + y;
			if (gx >= s.W || gy >= s.H) continue;
			const float c_mu = column_pass(s_row[BSR_PHOTOMETRIC_P_MU], x, y);
			const float c_e11 = column_pass(s_row[BSR_PHOTOMETRIC_P_E11], x, y);
			const float c_e12 = column_pass(s_row[BSR_PHOTOMETRIC_P_E12], x, y);
			const long long at = t.base + (long long)gy * s.W + gx;
			const float iv = img[at], tv = gt[at];
			const float diff = iv - tv;
			const float sg = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
			const float inner = (c_mu + (2.0f * iv) * c_e11) + tv * c_e12;
			grad[at] = gv * (kl * sg + ks * inner);
		}
		__syncthreads();
	}
}

// the checks both entry points share; fills the shape.  Returns 0 and s.tiles == 0 for an empty input.
static int loss_shape(const char* who, int B, int C, int H, int W, LossShape& s)
{
	if (B < 0 || C < 0 || H < 1 || W < 1) return fail("%s: need B, C >= 0 and H, W >= 1 (got %d, %d, %d, %d)", who, B, C, H, W);
	if ((long long)B * C * H >= (1LL << 31) || (long long)B * C * H * W >= (1LL << 31))
		return fail("%s: B * C * H * W must be below 2^31 (got %d * %d * %d * %d)", who, B, C, H, W);
	s.H = H;
	s.W = W;
	s.planes = (long long)B * C;
	s.tiles_x = ((long long)W + BSR_LOSS_TW - 1) / BSR_LOSS_TW;
	s.tiles_y = ((long long)H + BSR_LOSS_TH - 1) / BSR_LOSS_TH;
	s.tiles = s.planes * s.tiles_x * s.tiles_y;
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_photometric_scratch_bytes(int B, int C, int H, int W)
{
	if (B < 0 || C < 0 || H < 1 || W < 1) return 0;
	if ((long long)B * C * H >= (1LL << 31) || (long long)B * C * H * W >= (1LL << 31)) return 0;
	const long long tiles = (long long)B * C * (((long long)W + BSR_LOSS_TW - 1) / BSR_LOSS_TW) *
	                        (((long long)H + BSR_LOSS_TH - 1) / BSR_LOSS_TH);
	return align_up(BSR_LOSS_HEAD + (size_t)loss_blocks(tiles) * 2 * sizeof(double), 256);
}

int bsr_photometric_forward(int B, int C, int H, int W, const float* img, const float* gt, float lambda, float* partials,
                            float* ssim_map, float* out, void* scratch, void* stream)
{
	const char* who = "bsr_photometric_forward";
	LossShape s;
	if (loss_shape(who, B, C, H, W, s)) return 1;
	if (!out) return fail("%s: NULL out", who);
	if (((uintptr_t)img | (uintptr_t)gt | (uintptr_t)partials | (uintptr_t)ssim_map | (uintptr_t)out) & 3)
		return fail("%s: operands and outputs must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	if (s.tiles == 0) {
		if (hipMemsetAsync(out, 0, 3 * sizeof(float), st) != hipSuccess) return fail("%s: memset failed", who);
		return 0;
	}
	if (!img || !gt) return fail("%s: NULL operand", who);
	if (!scratch) return fail("%s: NULL scratch", who);
	if ((uintptr_t)scratch & 7) return fail("%s: scratch must be 8-byte aligned", who);
	const unsigned blocks = loss_blocks(s.tiles);
	LossScratch sc;
	sc.ticket = (unsigned*)scratch;
	sc.psum = (double*)((char*)scratch + BSR_LOSS_HEAD);
	if (hipMemsetAsync(sc.ticket, 0, sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	hipLaunchKernelGGL(k_photometric_fwd, dim3(blocks), dim3(BSR_LOSS_BLOCK), 0, st, s, img, gt, lambda, partials, ssim_map, out, sc);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_photometric_backward(int B, int C, int H, int W, const float* img, const float* gt, const float* partials,
                             float lambda, const float* g, float* grad, void* stream)
{
	const char* who = "bsr_photometric_backward";
	LossShape s;
	if (loss_shape(who, B, C, H, W, s)) return 1;
	if (s.tiles == 0) return 0;
	if (!img || !gt || !partials || !g || !grad) return fail("%s: NULL operand", who);
	if (((uintptr_t)img | (uintptr_t)gt | (uintptr_t)partials | (uintptr_t)g | (uintptr_t)grad) & 3)
		return fail("%s: operands and the gradient must be 4-byte aligned", who);
	const float n = (float)(s.planes * (long long)H * (long long)W);
	const float kl = (1.0f - lambda) / n, ks = -lambda / n;
	hipLaunchKernelGGL(k_photometric_bwd, dim3(loss_blocks(s.tiles)), dim3(BSR_LOSS_BLOCK), 0, (hipStream_t)stream, s, img, gt,
	                   partials, kl, ks, g, grad);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
