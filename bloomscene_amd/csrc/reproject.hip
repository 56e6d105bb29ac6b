// The point-cloud reprojection of the scene-lifting stage for gfx950 (include/bloomscene_reproject.h has the function,
// step by step; BloomScene.generate_pcd, bloomscene.py:428-656, "BS").
//
// bsr_warp_points:
//   k_warp_clear             the five sums and hit = 0, zmin = 0xffffffff.  A kernel and not hipMemsetAsync: replayed from a
//                            captured graph, memset nodes left the sums of the previous replay in place on the MI355X
//                            (mix_grid.hip met the same; docs/EXPERIMENTS.md)
//   k_warp_project           one thread per point: steps 1-3 -- pixel, hit, the atomic minimum of zf over the footprint
//   k_warp_splat             one thread per point: the projection again (the same inlined function, so the same bits),
//                            the z-test against the finished zmin, step 4's integer atomic adds
//   k_warp_finish            one workgroup per 32 x 16 pixel tile: steps 4 (resolve) to 7.  LDS holds hit with a halo of 10
//                            (4 dilation + 5 erosion + 1: mask_hf and the ring read a neighbour's mask), known with a halo
//                            of 6, mask with a halo of 1 and the resolved values with a halo of 5 (4 fill + 1 ring).
// WHY IT IS DETERMINISTIC.  zmin is an unsigned minimum, hit a store of 1, the sums integer adds: none depends on the
// order of its operands.  Everything after them is a function of one pixel's neighbourhood, evaluated in a fixed order.
// BOUNDS.  A footprint pixel is written only after x < W and y < H were tested (x0, y0 >= 0 follows from u, v >= 0);
// pixel[i] is in [0, H W) because 0 <= rint(u) <= W - 1 and 0 <= rint(v) <= H - 1; every LDS cell outside the frame is
// filled with the neutral value instead of a load.
//
// bsr_lift_count / bsr_lift_pixels: the ranks of a compaction (wg_scan.h) -- k_lift_count one count per 256 pixels,
// k_lift_scan their exclusive prefix in place by ONE workgroup (linear in the blocks) and the total; k_lift_pixels one thread
// per pixel, its row = its block's prefix + its rank in the block.
#include "common.h"
#include "wg_scan.h"
#include "../../include/bloomscene_reproject.h"

namespace bsr {

#define BSR_REPROJECT_BLOCK 256
#define BSR_WARP_TW 32
#define BSR_WARP_TH 16
#define BSR_WARP_FILL 4     // radius of the 9 x 9 window
#define BSR_WARP_ERODE 5    // radius of the 11 x 11 window
static_assert(BSR_REPROJECT_LIFT_BLOCK == BSR_REPROJECT_BLOCK, "one count per workgroup");

struct ReprojectCamera { double m[21]; };   // K or its inverse, R or its inverse, T: by value in the kernel-argument block

struct WarpPoint { bool valid; double u, v; float zf; };

#define BSR_REPROJECT_MAX_BLOCKS (1 << 16)   // grid-stride beyond 2^24 pixels
static unsigned pixel_blocks(size_t HW)
{
	const size_t nb = (HW + BSR_REPROJECT_BLOCK - 1) / BSR_REPROJECT_BLOCK;
	return (unsigned)(nb < BSR_REPROJECT_MAX_BLOCKS ? nb : BSR_REPROJECT_MAX_BLOCKS);
}

__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_warp_clear(size_t HW, unsigned long long* __restrict__ acc,
                                                                    uint32_t* __restrict__ zmin, unsigned char* __restrict__ hit)
{
	for (size_t q = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x; q < HW; q += (size_t)gridDim.x * BSR_REPROJECT_BLOCK) {
#pragma unroll
		for (int ch = 0; ch < 5; ch++) acc[ch * HW + q] = 0ull;
		zmin[q] = 0xffffffffu;
		hit[q] = 0;
	}
}

// P == 0: every output of a frame no point reaches
__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_warp_empty(size_t HW, float* __restrict__ image, float* __restrict__ depth,
                                                                    unsigned char* __restrict__ mask,
                                                                    unsigned char* __restrict__ mask_hf)
{
	for (size_t q = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x; q < HW; q += (size_t)gridDim.x * BSR_REPROJECT_BLOCK) {
		image[3 * q] = image[3 * q + 1] = image[3 * q + 2] = 0.0f;
		depth[q] = 0.0f;
		mask[q] = mask_hf[q] = 0;
	}
}

// step 1 (the header's order; the unit is built without contraction)
__device__ __forceinline__ WarpPoint warp_project(const ReprojectCamera& cam, const float* __restrict__ points, long long ps,
                                                  long long cs, const float* __restrict__ colors, size_t i, int H, int W)
{
	const double* K = cam.m;
	const double* R = cam.m + 9;
	const double* T = cam.m + 18;
	const float* p = points + (long long)i * ps;
	const double x0 = (double)p[0], x1 = (double)p[cs], x2 = (double)p[2 * cs];
	double c[3], q[3];
#pragma unroll
	for (int j = 0; j < 3; j++) c[j] = ((R[3 * j] * x0 + R[3 * j + 1] * x1) + R[3 * j + 2] * x2) + T[j];
#pragma unroll
	for (int j = 0; j < 3; j++) q[j] = (K[3 * j] * c[0] + K[3 * j + 1] * c[1]) + K[3 * j + 2] * c[2];
	WarpPoint r;
	r.u = q[0] / q[2];
	r.v = q[1] / q[2];
	r.zf = (float)q[2];
	const float cr = colors[3 * i], cg = colors[3 * i + 1], cb = colors[3 * i + 2];
	r.valid = q[2] > 0.0 && r.u >= 0.0 && r.u <= (double)(W - 1) && r.v >= 0.0 && r.v <= (double)(H - 1) &&
	          __builtin_isfinite(cr) && __builtin_isfinite(cg) && __builtin_isfinite(cb);
	return r;
}

// the footprint of step 3: pixel k of a valid point and its weight; false: not part of it
__device__ __forceinline__ bool warp_corner(const WarpPoint& p, int k, int H, int W, int& q, double& w)
{
	const double fx0 = __builtin_floor(p.u), fy0 = __builtin_floor(p.v);
	const double fx = p.u - fx0, fy = p.v - fy0;
	const int x = (int)fx0 + (k & 1), y = (int)fy0 + (k >> 1);
	w = ((k & 1) ? fx : 1.0 - fx) * ((k >> 1) ? fy : 1.0 - fy);
	const bool in = w > 0.0 && x >= 0 && y >= 0 && x < W && y < H;
	q = in ? y * W + x : 0;   // (only inside the frame: y * W + x fits an int there)
	return in;
}

__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_warp_project(int P, int H, int W, ReprojectCamera cam,
                                                                      const float* __restrict__ points, long long ps,
                                                                      long long cs, const float* __restrict__ colors,
                                                                      int* __restrict__ pixel, uint32_t* zmin,
                                                                      unsigned char* hit)
{
	const size_t i = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x;
	if (i >= (size_t)P) return;
	const WarpPoint p = warp_project(cam, points, ps, cs, colors, i, H, W);
	if (!p.valid) {
		pixel[i] = -1;
		return;
	}
	const int pix = (int)__builtin_rint(p.v) * W + (int)__builtin_rint(p.u);
	pixel[i] = pix;
	hit[pix] = 1;
	const uint32_t zb = __float_as_uint(p.zf);
#pragma unroll
	for (int k = 0; k < 4; k++) {
		int q;
		double w;
		if (warp_corner(p, k, H, W, q, w)) atomicMin(zmin + q, zb);
	}
}

// one contribution of step 4
__device__ __forceinline__ void warp_contribute(unsigned long long* acc, double w, double x)
{
	double t = w * x * 268435456.0;   // 2^BSR_REPROJECT_SHIFT
	t = t < -4611686018427387904.0 ? -4611686018427387904.0 : (t > 4611686018427387904.0 ? 4611686018427387904.0 : t);
	const long long v = (long long)__builtin_rint(t);
	if (v != 0) atomicAdd(acc, (unsigned long long)v);
}
static_assert(BSR_REPROJECT_SHIFT == 28, "the constant of warp_contribute");

__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_warp_splat(int P, int H, int W, ReprojectCamera cam,
                                                                    const float* __restrict__ points, long long ps,
                                                                    long long cs, const float* __restrict__ colors,
                                                                    int use_z_test, double one_tol,
                                                                    const uint32_t* __restrict__ zmin,
                                                                    unsigned long long* acc)
{
	const size_t i = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x;
	if (i >= (size_t)P) return;
	const WarpPoint p = warp_project(cam, points, ps, cs, colors, i, H, W);
	if (!p.valid) return;
	const size_t HW = (size_t)H * W;
	const double x[5] = {1.0, (double)colors[3 * i], (double)colors[3 * i + 1], (double)colors[3 * i + 2], (double)p.zf};
#pragma unroll
	for (int k = 0; k < 4; k++) {
		int q;
		double w;
		if (!warp_corner(p, k, H, W, q, w)) continue;
		if (use_z_test && !((double)p.zf <= (double)__uint_as_float(zmin[q]) * one_tol)) continue;
#pragma unroll
		for (int ch = 0; ch < 5; ch++) warp_contribute(acc + ch * HW + q, w, x[ch]);
	}
}

#define BSR_WARP_HIT_HALO (BSR_WARP_FILL + BSR_WARP_ERODE + 1)   // 10
#define BSR_WARP_KNOWN_HALO (BSR_WARP_ERODE + 1)                 // 6
#define BSR_WARP_VAL_HALO (BSR_WARP_FILL + 1)                    // 5
#define BSR_WARP_HIT_W (BSR_WARP_TW + 2 * BSR_WARP_HIT_HALO)
#define BSR_WARP_HIT_H (BSR_WARP_TH + 2 * BSR_WARP_HIT_HALO)
#define BSR_WARP_KNOWN_W (BSR_WARP_TW + 2 * BSR_WARP_KNOWN_HALO)
#define BSR_WARP_KNOWN_H (BSR_WARP_TH + 2 * BSR_WARP_KNOWN_HALO)
#define BSR_WARP_VAL_W (BSR_WARP_TW + 2 * BSR_WARP_VAL_HALO)
#define BSR_WARP_VAL_H (BSR_WARP_TH + 2 * BSR_WARP_VAL_HALO)
#define BSR_WARP_THREADS (BSR_WARP_TW * BSR_WARP_TH)

__global__ void __launch_bounds__(BSR_WARP_THREADS) k_warp_finish(int H, int W, int use_z_test, double one_tol,
                                                                  const long long* __restrict__ acc,
                                                                  const unsigned char* __restrict__ hit,
                                                                  float* __restrict__ image, float* __restrict__ depth,
                                                                  unsigned char* __restrict__ mask,
                                                                  unsigned char* __restrict__ mask_hf)
{
	__shared__ unsigned char s_hit[BSR_WARP_HIT_H][BSR_WARP_HIT_W];
	__shared__ unsigned char s_known[BSR_WARP_KNOWN_H][BSR_WARP_KNOWN_W];
	__shared__ unsigned char s_mask[BSR_WARP_TH + 2][BSR_WARP_TW + 2];
	__shared__ unsigned char s_res[BSR_WARP_VAL_H][BSR_WARP_VAL_W];
	__shared__ float s_val[4][BSR_WARP_VAL_H][BSR_WARP_VAL_W];   // r, g, b, depth of the resolved pixels
	const int tid = threadIdx.x;
	const int tx0 = blockIdx.x * BSR_WARP_TW, ty0 = blockIdx.y * BSR_WARP_TH;
	const size_t HW = (size_t)H * W;

	// hit (0 outside the frame: neutral for the maximum) and the resolved values of step 4
	for (int t = tid; t < BSR_WARP_HIT_H * BSR_WARP_HIT_W; t += BSR_WARP_THREADS) {
		const int ly = t / BSR_WARP_HIT_W, lx = t - ly * BSR_WARP_HIT_W;
		const int gy = ty0 - BSR_WARP_HIT_HALO + ly, gx = tx0 - BSR_WARP_HIT_HALO + lx;
		s_hit[ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? hit[(size_t)gy * W + gx] : (unsigned char)0;
	}
	for (int t = tid; t < BSR_WARP_VAL_H * BSR_WARP_VAL_W; t += BSR_WARP_THREADS) {
		const int ly = t / BSR_WARP_VAL_W, lx = t - ly * BSR_WARP_VAL_W;
		const int gy = ty0 - BSR_WARP_VAL_HALO + ly, gx = tx0 - BSR_WARP_VAL_HALO + lx;
		unsigned char res = 0;
		float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
		if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
			const size_t q = (size_t)gy * W + gx;
			const long long sw = acc[q];
			if (sw > 0) {
				res = 1;
#pragma unroll
				for (int ch = 0; ch < 4; ch++) v[ch] = (float)((double)acc[(ch + 1) * HW + q] / (double)sw);
			}
		}
		s_res[ly][lx] = res;
#pragma unroll
		for (int ch = 0; ch < 4; ch++) s_val[ch][ly][lx] = v[ch];
	}
	__syncthreads();
	// known: the 9 x 9 maximum of hit (1 outside the frame: neutral for the minimum that follows)
	for (int t = tid; t < BSR_WARP_KNOWN_H * BSR_WARP_KNOWN_W; t += BSR_WARP_THREADS) {
		const int ly = t / BSR_WARP_KNOWN_W, lx = t - ly * BSR_WARP_KNOWN_W;
		const int gy = ty0 - BSR_WARP_KNOWN_HALO + ly, gx = tx0 - BSR_WARP_KNOWN_HALO + lx;
		unsigned char k = 1;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
			k = 0;   // s_hit row of gy - 4 is ly (10 - 6 - 4 = 0)
			for (int dy = 0; dy <= 2 * BSR_WARP_FILL; dy++)
				for (int dx = 0; dx <= 2 * BSR_WARP_FILL; dx++) k |= s_hit[ly + dy][lx + dx];
		}
		s_known[ly][lx] = k;
	}
	__syncthreads();
	// mask: the 11 x 11 minimum of known
	for (int t = tid; t < (BSR_WARP_TH + 2) * (BSR_WARP_TW + 2); t += BSR_WARP_THREADS) {
		const int ly = t / (BSR_WARP_TW + 2), lx = t - ly * (BSR_WARP_TW + 2);
		const int gy = ty0 - 1 + ly, gx = tx0 - 1 + lx;
		unsigned char m = 0;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
			m = 1;   // s_known row of gy - 5 is ly (6 - 1 - 5 = 0)
			for (int dy = 0; dy <= 2 * BSR_WARP_ERODE; dy++)
				for (int dx = 0; dx <= 2 * BSR_WARP_ERODE; dx++) m &= s_known[ly + dy][lx + dx];
		}
		s_mask[ly][lx] = m;
	}
	__syncthreads();

	const int c = tx0 + (tid & (BSR_WARP_TW - 1)), r = ty0 + tid / BSR_WARP_TW;
	if (r >= H || c >= W) return;
	// step 6: the pixel whose value this one shows
	const int sr = r < 1 ? 1 : (r > H - 2 ? H - 2 : r), sc = c < 1 ? 1 : (c > W - 2 ? W - 2 : c);
	const int vy = sr - ty0 + BSR_WARP_VAL_HALO, vx = sc - tx0 + BSR_WARP_VAL_HALO;
	float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
	if (s_res[vy][vx]) {
#pragma unroll
		for (int ch = 0; ch < 4; ch++) v[ch] = s_val[ch][vy][vx];
	} else if (s_known[sr - ty0 + BSR_WARP_KNOWN_HALO][sc - tx0 + BSR_WARP_KNOWN_HALO]) {
		// step 5 around (sr, sc), the window clipped to the frame (it lies within the halo of 5: |sr - r|, |sc - c| <= 1)
		const int y0 = sr - BSR_WARP_FILL < 0 ? 0 : sr - BSR_WARP_FILL, y1 = sr + BSR_WARP_FILL > H - 1 ? H - 1 : sr + BSR_WARP_FILL;
		const int x0 = sc - BSR_WARP_FILL < 0 ? 0 : sc - BSR_WARP_FILL, x1 = sc + BSR_WARP_FILL > W - 1 ? W - 1 : sc + BSR_WARP_FILL;
		bool any = false;
		float dmin = 0.0f;
		for (int y = y0; y <= y1; y++)
			for (int x = x0; x <= x1; x++) {
				const int ly = y - ty0 + BSR_WARP_VAL_HALO, lx = x - tx0 + BSR_WARP_VAL_HALO;
				if (!s_res[ly][lx]) continue;
				const float d = s_val[3][ly][lx];
				dmin = (!any || d < dmin) ? d : dmin;
				any = true;
			}
		const double lim = one_tol * (double)dmin;
		double s[4] = {0.0, 0.0, 0.0, 0.0}, sw = 0.0;
		for (int y = y0; y <= y1; y++)
			for (int x = x0; x <= x1; x++) {
				const int ly = y - ty0 + BSR_WARP_VAL_HALO, lx = x - tx0 + BSR_WARP_VAL_HALO;
				if (!s_res[ly][lx]) continue;
				if (use_z_test && !((double)s_val[3][ly][lx] <= lim)) continue;
				const double g = 1.0 / (double)((y - sr) * (y - sr) + (x - sc) * (x - sc));   // (never the centre: it is not resolved)
#pragma unroll
				for (int ch = 0; ch < 4; ch++) s[ch] = s[ch] + g * (double)s_val[ch][ly][lx];
				sw = sw + g;
			}
		if (sw > 0.0) {
#pragma unroll
			for (int ch = 0; ch < 4; ch++) v[ch] = (float)(s[ch] / sw);
		}
	}
	// step 7
	const int my = r - ty0 + 1, mx = c - tx0 + 1;
	const unsigned char m = s_mask[my][mx];
	const size_t q = (size_t)r * W + c;
	image[3 * q] = m ? v[0] : 0.0f;
	image[3 * q + 1] = m ? v[1] : 0.0f;
	image[3 * q + 2] = m ? v[2] : 0.0f;
	depth[q] = v[3];
	mask[q] = m;
	const int hy = (r < H - 2 ? r : H - 2) - ty0 + 1, hx = (c < W - 2 ? c : W - 2) - tx0 + 1;   // (>= 0: at most one back)
	const unsigned char m0 = s_mask[hy][hx];
	mask_hf[q] = (unsigned char)((m0 != s_mask[hy + 1][hx]) || (m0 != s_mask[hy][hx + 1]));
}

// ---- lift ----

__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_lift_count(int HW, const unsigned char* __restrict__ select,
                                                                    uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_wave[BSR_REPROJECT_BLOCK / 64];
	const size_t i = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x;
	uint32_t n;
	wg_exclusive_count<BSR_REPROJECT_BLOCK / 64>(i < (size_t)HW && select[i] != 0, s_wave, n);
	if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// counts[b] -> the selected pixels before block b, in place; *total = all of them.  ONE workgroup: linear in the blocks
#define BSR_LIFT_SCAN_WAVES 16
__global__ void __launch_bounds__(64 * BSR_LIFT_SCAN_WAVES) k_lift_scan(int blocks, uint32_t* counts, unsigned* __restrict__ total)
{
	__shared__ uint32_t s_wave[2 * BSR_LIFT_SCAN_WAVES];
	const uint32_t all = wg_exclusive_scan<BSR_LIFT_SCAN_WAVES, 4>(blocks, counts, s_wave, true);
	if (threadIdx.x == 0) *total = all;
}

__global__ void __launch_bounds__(BSR_REPROJECT_BLOCK) k_lift_pixels(int HW, int W, ReprojectCamera cam,
                                                                     const float* __restrict__ depth,
                                                                     const float* __restrict__ image_f,
                                                                     const unsigned char* __restrict__ image_b,
                                                                     const unsigned char* __restrict__ select,
                                                                     const uint32_t* __restrict__ before, int n,
                                                                     float* __restrict__ points, float* __restrict__ colors)
{
	__shared__ uint32_t s_wave[BSR_REPROJECT_BLOCK / 64];
	const size_t i = (size_t)blockIdx.x * BSR_REPROJECT_BLOCK + threadIdx.x;
	const bool in = i < (size_t)HW;
	size_t row = i;
	bool take = in;
	if (select) {   // (uniform)
		take = in && select[i] != 0;
		row = (size_t)before[blockIdx.x] + wg_exclusive_count<BSR_REPROJECT_BLOCK / 64>(take, s_wave);
	}
	if (!take || row >= (size_t)n) return;
	const double* Ki = cam.m;
	const double* Ri = cam.m + 9;
	const double* T = cam.m + 18;
	const int r = (int)(i / (size_t)W), c = (int)(i - (size_t)r * W);
	const float d = depth[i];
	const double a0 = (double)((float)c * d), a1 = (double)((float)r * d), a2 = (double)d;
	double t[3];
#pragma unroll
	for (int j = 0; j < 3; j++) t[j] = ((Ki[3 * j] * a0 + Ki[3 * j + 1] * a1) + Ki[3 * j + 2] * a2) - T[j];
#pragma unroll
	for (int j = 0; j < 3; j++) points[3 * row + j] = (float)((Ri[3 * j] * t[0] + Ri[3 * j + 1] * t[1]) + Ri[3 * j + 2] * t[2]);
#pragma unroll
	for (int j = 0; j < 3; j++) colors[3 * row + j] = image_f ? image_f[3 * i + j] : (float)image_b[3 * i + j] / 255.0f;
}

static bool frame_ok(int H, int W, int least) { return H >= least && W >= least && (long long)H * W < 0x80000000LL; }

static ReprojectCamera camera_of(const double* camera)
{
	ReprojectCamera c;
	for (int k = 0; k < 21; k++) c.m[k] = camera[k];
	return c;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_reproject_scratch_bytes(int H, int W)
{
	if (!frame_ok(H, W, 3)) return 0;
	return align_up((size_t)H * W * (5 * 8 + 4 + 1), 256);
}

int bsr_warp_points(int P, int H, int W, const float* points, long long point_stride, long long comp_stride,
                    const float* colors, const double* camera, int use_z_test, double z_tolerance, float* image,
                    float* depth, unsigned char* mask, unsigned char* mask_hf, int* pixel, void* scratch, void* stream)
{
	const char* who = "bsr_warp_points";
	if (P < 0) return fail("%s: need P >= 0 (got %d)", who, P);
	if (!frame_ok(H, W, 3)) return fail("%s: need H, W >= 3 and H * W below 2^31 (got %d, %d)", who, H, W);
	if (use_z_test && !(z_tolerance >= 0.0 && z_tolerance <= 1.7976931348623157e308))
		return fail("%s: z_tolerance must be finite and >= 0 (got %g)", who, z_tolerance);
	if (!image || !depth || !mask || !mask_hf) return fail("%s: NULL output", who);
	if (((uintptr_t)image | (uintptr_t)depth) & 3) return fail("%s: image and depth must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const size_t HW = (size_t)H * W;
	if (P == 0) {
		hipLaunchKernelGGL(k_warp_empty, dim3(pixel_blocks(HW)), dim3(BSR_REPROJECT_BLOCK), 0, st, HW, image, depth, mask, mask_hf);
		if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
		return 0;
	}
	if (!points || !colors || !camera || !pixel || !scratch) return fail("%s: NULL buffer", who);
	if (((uintptr_t)points | (uintptr_t)colors | (uintptr_t)pixel) & 3)
		return fail("%s: points, colors and pixel must be 4-byte aligned", who);
	if ((uintptr_t)scratch & 7) return fail("%s: scratch must be 8-byte aligned", who);
	unsigned long long* acc = (unsigned long long*)scratch;
	uint32_t* zmin = (uint32_t*)(acc + 5 * HW);
	unsigned char* hit = (unsigned char*)(zmin + HW);
	hipLaunchKernelGGL(k_warp_clear, dim3(pixel_blocks(HW)), dim3(BSR_REPROJECT_BLOCK), 0, st, HW, acc, zmin, hit);
	const ReprojectCamera cam = camera_of(camera);
	const double one_tol = 1.0 + (use_z_test ? z_tolerance : 0.0);
	const dim3 blk(BSR_REPROJECT_BLOCK), grid((unsigned)(((size_t)P + BSR_REPROJECT_BLOCK - 1) / BSR_REPROJECT_BLOCK));
	hipLaunchKernelGGL(k_warp_project, grid, blk, 0, st, P, H, W, cam, points, point_stride, comp_stride, colors, pixel, zmin,
	                   hit);
	hipLaunchKernelGGL(k_warp_splat, grid, blk, 0, st, P, H, W, cam, points, point_stride, comp_stride, colors, use_z_test,
	                   one_tol, (const uint32_t*)zmin, acc);
	const dim3 tiles((unsigned)((W + BSR_WARP_TW - 1) / BSR_WARP_TW), (unsigned)((H + BSR_WARP_TH - 1) / BSR_WARP_TH));
	hipLaunchKernelGGL(k_warp_finish, tiles, dim3(BSR_WARP_THREADS), 0, st, H, W, use_z_test, one_tol, (const long long*)acc,
	                   (const unsigned char*)hit, image, depth, mask, mask_hf);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

size_t bsr_lift_scratch_bytes(int H, int W)
{
	if (!frame_ok(H, W, 1)) return 0;
	return align_up((((size_t)H * W + BSR_REPROJECT_BLOCK - 1) / BSR_REPROJECT_BLOCK) * 4, 256);
}

int bsr_lift_count(int H, int W, const unsigned char* select, void* scratch, unsigned* total, void* stream)
{
	const char* who = "bsr_lift_count";
	if (!frame_ok(H, W, 1)) return fail("%s: need H, W >= 1 and H * W below 2^31 (got %d, %d)", who, H, W);
	if (!select || !scratch || !total) return fail("%s: NULL buffer", who);
	if (((uintptr_t)scratch | (uintptr_t)total) & 3) return fail("%s: scratch and total must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const size_t HW = (size_t)H * W;
	const unsigned blocks = (unsigned)((HW + BSR_REPROJECT_BLOCK - 1) / BSR_REPROJECT_BLOCK);
	hipLaunchKernelGGL(k_lift_count, dim3(blocks), dim3(BSR_REPROJECT_BLOCK), 0, st, (int)HW, select, (uint32_t*)scratch);
	hipLaunchKernelGGL(k_lift_scan, dim3(1), dim3(64 * BSR_LIFT_SCAN_WAVES), 0, st, (int)blocks, (uint32_t*)scratch, total);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_lift_pixels(int H, int W, const float* depth, const float* image_f, const unsigned char* image_b,
                    const double* camera, const unsigned char* select, const void* scratch, int n, float* points,
                    float* colors, void* stream)
{
	const char* who = "bsr_lift_pixels";
	if (!frame_ok(H, W, 1)) return fail("%s: need H, W >= 1 and H * W below 2^31 (got %d, %d)", who, H, W);
	const size_t HW = (size_t)H * W;
	if (n < 0 || (size_t)n > HW) return fail("%s: need 0 <= n <= H * W (got %d)", who, n);
	if (!select && (size_t)n != HW) return fail("%s: without a selection n must be H * W (got %d)", who, n);
	if (n == 0) return 0;
	if (!depth || !camera || !points || !colors) return fail("%s: NULL buffer", who);
	if ((image_f != NULL) == (image_b != NULL)) return fail("%s: exactly one of image_f and image_b must be given", who);
	if (select && !scratch) return fail("%s: a selection needs the scratch of bsr_lift_count", who);
	if (((uintptr_t)depth | (uintptr_t)image_f | (uintptr_t)scratch | (uintptr_t)points | (uintptr_t)colors) & 3)
		return fail("%s: depth, image_f, scratch, points and colors must be 4-byte aligned", who);
	hipLaunchKernelGGL(k_lift_pixels, dim3((unsigned)((HW + BSR_REPROJECT_BLOCK - 1) / BSR_REPROJECT_BLOCK)),
	                   dim3(BSR_REPROJECT_BLOCK), 0, (hipStream_t)stream, (int)HW, W, camera_of(camera), depth, image_f, image_b,
	                   select, (const uint32_t*)scratch, n, points, colors);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
