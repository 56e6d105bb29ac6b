// The three anchor MLP heads of generate_neural_gaussians for gfx950 (include/bloomscene_heads.h): mlp_opacity, mlp_cov and
// mlp_color on the visible anchors, with the view geometry, the reshapes and the offset mask folded in.
//
//   k_heads_fwd        X -> hid -> pre2 -> the three outputs, one head after the other
//   k_heads_bwd_rows   recomputes hid, forms dpre2 / dpre1 / dX per row -> d feat, d anchor, d offset_mask; with a weight
//                      gradient asked for it also leaves X, hid, dpre1, dpre2 of every row in the scratch
//   k_mlp_wgrad, k_mlp_wsum (mlp_wgrad.h)   the weight gradients from that scratch: heads_segments, heads_products
//
// LANE MAPPING (forward and row pass).  A lane is an anchor row; a workgroup is ONE wave of 64 rows.  The row's vectors
// that are indexed by a loop variable (X, hid, dpre2, dX) live in LDS as [index][lane] with a pitch of 65 floats: the
// lane's own column is read without bank conflicts, and the cooperative, coalesced loads and stores of whole rows walk it
// with a stride of 65 (conflict-free as well).  Eight outputs are accumulated at a time in registers; their weights are
// uniform over the wave: a block of 8 x 8 of them is one coalesced vector load, and each FMA takes its weight from a lane
// of it as a scalar operand (mlp_rows.h, which holds these products: THE WEIGHTS OF A STEP), with one LDS read per eight
// FMAs.  Every chain is written with explicit fmaf in the order the header states: the build stays at -ffp-contract=off.
// WEIGHT GRADIENTS.  The reduction index is the row, which the row pass has on the lane; so that pass stores its per-row
// operands (row-major, rows padded to 16 bytes) and k_mlp_wgrad runs dW = dpre^T X as a register-blocked product: a
// thread owns a 4 x 4 block of one weight matrix and walks its range of rows in order, two 16-byte loads per 16 FMAs
// (fp64 ones: the sums over rows are the one place where fp32 accumulation in a fixed order loses to a library's tree).
// The grid is a function of (n, F, K) alone.
#include "common.h"
#include "lds_reserve.h"
#include "mlp_rows.h"   // uload, lane_value, step_fma, chain_rows, dot_cols, coop_store, coop_zero, store_block, the activations
#include "mlp_wgrad.h"
#include "../../include/bloomscene_heads.h"

namespace bsr {

#define HEADS_T MLP_ROWS_T     // rows a workgroup (one wave)
#define HEADS_P MLP_ROWS_P     // LDS pitch of a [index][lane] vector
#define HEADS_NJ MLP_ROWS_NJ   // outputs accumulated at a time

struct HeadsArgs {
	int n, F, K;
	const float* feat;
	long long fs;
	const float *anchor, *cam, *mask;
	bsr_heads_weights w;
};

__host__ __device__ __forceinline__ int heads_outputs(int h, int K) { return h == 0 ? K : (h == 1 ? 7 * K : 3 * K); }
__host__ __device__ __forceinline__ int heads_offset(int h, int K) { return h == 0 ? 0 : (h == 1 ? K : 8 * K); }

// Element order of a partial: W1 of the three heads [3 F, F + 4], b1 [3 F], W2 [11 K, F], b2 [11 K], each cut by head.
static MlpSegments heads_segments(int F, int K, const bsr_heads_weight_grads* dw)
{
	const bsr_heads_weight_grads g = dw ? *dw : bsr_heads_weight_grads{};
	MlpSegments d = {};
	for (int h = 0; h < 3; h++) d.add(F * (F + 4), g.head[h].w1);
	for (int h = 0; h < 3; h++) d.add(F, g.head[h].b1);
	for (int h = 0; h < 3; h++) d.add(heads_outputs(h, K) * F, g.head[h].w2);
	for (int h = 0; h < 3; h++) d.add(heads_outputs(h, K), g.head[h].b2);
	return d;
}

// layer 1 of the three heads as ONE stacked product over the shared X, layer 2 head by head
static MlpProducts heads_products(int F, int K, const MlpRowScratch& rs, const MlpSegments& d)
{
	MlpProducts p = {};
	p.add(rs.dp1, rs.ldh, rs.x, rs.ldx, 3 * F, F + 4, d, 0, 3);
	for (int h = 0; h < 3; h++)
		p.add(rs.dp2 + heads_offset(h, K), rs.ld2, rs.hid + h * F, rs.ldh, heads_outputs(h, K), F, d, 6 + h, 9 + h);
	return p;
}

// x [F + 4], hid / dp1 [3 F], dp2 [11 K]
static MlpWgradLayout heads_layout(int n, int F, int K) { return mlp_wgrad_layout(n, F + 4, 3 * F, 11 * K, heads_segments(F, K, nullptr).tot); }

static bool heads_shape_ok(int n, int F, int K)
{
	if (n < 0 || F < 1 || F > BSR_HEADS_MAX_F || K < 1 || K > BSR_HEADS_MAX_K) return false;
	const long long widest = 7 * K > F + 4 ? 7 * K : F + 4;
	return (long long)n * widest < (1LL << 31);
}

// X of the workgroup's rows -> Xs [F + 4][lane]; rows past n are zeros.  Returns nothing: v and dist are read back
// from Xs where needed.
__device__ __forceinline__ void stage_x(const HeadsArgs& a, float* Xs, long long row0, int rows, int lane)
{
	const int F = a.F;
	for (int idx = lane; idx < HEADS_T * F; idx += HEADS_T) {
		const int r = idx / F, k = idx - r * F;
		Xs[k * HEADS_P + r] = r < rows ? a.feat[(row0 + r) * a.fs + k] : 0.0f;
	}
	float vx = 0.0f, vy = 0.0f, vz = 0.0f, dist = 0.0f;
	if (lane < rows) {
		const float* p = a.anchor + (row0 + lane) * 3;
		const float dx = p[0] - uload(a.cam, 0), dy = p[1] - uload(a.cam, 1), dz = p[2] - uload(a.cam, 2);
		dist = sqrtf((dx * dx + dy * dy) + dz * dz);
		vx = dx / dist;
		vy = dy / dist;
		vz = dz / dist;
	}
	Xs[(F + 0) * HEADS_P + lane] = vx;
	Xs[(F + 1) * HEADS_P + lane] = vy;
	Xs[(F + 2) * HEADS_P + lane] = vz;
	Xs[(F + 3) * HEADS_P + lane] = dist;
}

__global__ void __launch_bounds__(HEADS_T) k_heads_fwd(HeadsArgs a, float* __restrict__ opacity, float* __restrict__ color,
                                                       float* __restrict__ scale_rot, float* __restrict__ maps)
{
	extern __shared__ float heads_lds[];
	const int F = a.F, K = a.K, Kd = F + 4, lane = threadIdx.x;
	float* Xs = heads_lds;
	float* Hs = Xs + Kd * HEADS_P;
	const long long row0 = (long long)blockIdx.x * HEADS_T, row = row0 + lane;
	const long long left = (long long)a.n - row0;
	const int rows = left < HEADS_T ? (int)left : HEADS_T;
	const bool valid = lane < rows;
	stage_x(a, Xs, row0, rows, lane);
	__syncthreads();
	float* pre1 = maps ? maps + (size_t)row * (3 * F) : nullptr;
	float* pre2 = maps ? maps + (size_t)a.n * (3 * F) + (size_t)row * (11 * K) : nullptr;
	float acc[HEADS_NJ];
	for (int h = 0; h < 3; h++) {
		const float *w1 = a.w.head[h].w1, *b1 = a.w.head[h].b1, *w2 = a.w.head[h].w2, *b2 = a.w.head[h].b2;
		const int O = heads_outputs(h, K), off = heads_offset(h, K);
		for (int j0 = 0; j0 < F; j0 += HEADS_NJ) {
			chain_rows(w1, b1, F, Kd, j0, Xs + lane, acc, lane);
#pragma unroll
			for (int jj = 0; jj < HEADS_NJ; jj++)
				if (j0 + jj < F) {
					if (maps && valid) pre1[h * F + j0 + jj] = acc[jj];
					Hs[(j0 + jj) * HEADS_P + lane] = mlp_relu(acc[jj]);
				}
		}
		__syncthreads();
		float* out = (h == 0 ? opacity : (h == 1 ? scale_rot : color)) + (size_t)row * O;
		for (int o0 = 0; o0 < O; o0 += HEADS_NJ) {
			chain_rows(w2, b2, O, F, o0, Hs + lane, acc, lane);
			if (!valid) continue;
			const int count = O - o0;
			if (maps) {
#pragma unroll
				for (int jj = 0; jj < HEADS_NJ; jj++)
					if (jj < count) pre2[off + o0 + jj] = acc[jj];
			}
			if (h == 0) {
#pragma unroll
				for (int jj = 0; jj < HEADS_NJ; jj++) {
					const float t = mlp_tanh(acc[jj]);
					acc[jj] = a.mask && jj < count ? t * a.mask[(size_t)row * K + o0 + jj] : t;
				}
			} else if (h == 2) {
#pragma unroll
				for (int jj = 0; jj < HEADS_NJ; jj++) acc[jj] = mlp_sigmoid(acc[jj]);
			}
			store_block(out + o0, acc, count);
		}
		__syncthreads();   // (Hs is the next head's)
	}
}

__global__ void __launch_bounds__(HEADS_T) k_heads_bwd_rows(HeadsArgs a, const float* __restrict__ color,
                                                            const float* __restrict__ g_o, const float* __restrict__ g_c,
                                                            const float* __restrict__ g_s, float* __restrict__ d_feat,
                                                            float* __restrict__ d_anchor, float* __restrict__ d_mask,
                                                            MlpRowScratch rs)
{
	extern __shared__ float heads_lds[];
	const int F = a.F, K = a.K, Kd = F + 4, lane = threadIdx.x;
	float* Xs = heads_lds;
	float* Hs = Xs + Kd * HEADS_P;
	float* Ds = Hs + F * HEADS_P;
	float* dXs = Ds + 7 * K * HEADS_P;
	const long long row0 = (long long)blockIdx.x * HEADS_T, row = row0 + lane;
	const long long left = (long long)a.n - row0;
	const int rows = left < HEADS_T ? (int)left : HEADS_T;
	const bool valid = lane < rows;
	const bool sums = rs.x != nullptr;
	stage_x(a, Xs, row0, rows, lane);
	__syncthreads();
	if (sums) coop_store(rs.x + (size_t)row0 * rs.ldx, rs.ldx, Kd, Xs, rows, lane);
	float acc[HEADS_NJ];
	bool first = true;
	for (int h = 0; h < 3; h++) {
		const float* g = h == 0 ? g_o : (h == 1 ? g_s : g_c);
		const int O = heads_outputs(h, K), off = heads_offset(h, K);
		if (!g) {   // a head without upstream is left out: nothing enters dX, and its operands for the weight sums are zeros
			if (h == 0 && d_mask && valid)
				for (int o = 0; o < K; o++) d_mask[(size_t)row * K + o] = 0.0f;
			if (sums) {
				coop_zero(rs.hid + (size_t)row0 * rs.ldh + h * F, rs.ldh, F, rows, lane);
				coop_zero(rs.dp1 + (size_t)row0 * rs.ldh + h * F, rs.ldh, F, rows, lane);
				coop_zero(rs.dp2 + (size_t)row0 * rs.ld2 + off, rs.ld2, O, rows, lane);
			}
			continue;
		}
		const float *w1 = a.w.head[h].w1, *b1 = a.w.head[h].b1, *w2 = a.w.head[h].w2, *b2 = a.w.head[h].b2;
		for (int j0 = 0; j0 < F; j0 += HEADS_NJ) {
			chain_rows(w1, b1, F, Kd, j0, Xs + lane, acc, lane);
#pragma unroll
			for (int jj = 0; jj < HEADS_NJ; jj++)
				if (j0 + jj < F) Hs[(j0 + jj) * HEADS_P + lane] = mlp_relu(acc[jj]);
		}
		__syncthreads();
		if (sums) coop_store(rs.hid + (size_t)row0 * rs.ldh + h * F, rs.ldh, F, Hs, rows, lane);
		if (h == 0) {
			for (int o0 = 0; o0 < O; o0 += HEADS_NJ) {
				chain_rows(w2, b2, O, F, o0, Hs + lane, acc, lane);
#pragma unroll
				for (int jj = 0; jj < HEADS_NJ; jj++) {
					const int o = o0 + jj;
					if (o < O) {
						const float t = mlp_tanh(acc[jj]);
						const float m = a.mask && valid ? a.mask[(size_t)row * K + o] : 1.0f;
						const float go = valid ? g[(size_t)row * K + o] : 0.0f;
						if (d_mask && valid) d_mask[(size_t)row * K + o] = go * t;
						Ds[o * HEADS_P + lane] = (go * m) * (1.0f - t * t);
					}
				}
			}
		} else {
			const size_t at = (size_t)row0 * O;
			for (int idx = lane; idx < HEADS_T * O; idx += HEADS_T) {
				const int r = idx / O, o = idx - r * O;
				float v = 0.0f;
				if (r < rows) {
					v = g[at + idx];
					if (h == 2) {
						const float s = color[at + idx];
						v = (v * s) * (1.0f - s);
					}
				}
				Ds[o * HEADS_P + r] = v;
			}
		}
		__syncthreads();
		if (sums) coop_store(rs.dp2 + (size_t)row0 * rs.ld2 + off, rs.ld2, O, Ds, rows, lane);
		for (int j0 = 0; j0 < F; j0 += HEADS_NJ) {
			dot_cols(w2, O, F, j0, Ds + lane, acc, lane);
#pragma unroll
			for (int jj = 0; jj < HEADS_NJ; jj++)
				if (j0 + jj < F) {
					float* p = &Hs[(j0 + jj) * HEADS_P + lane];
					*p = *p > 0.0f ? acc[jj] : 0.0f;   // hid -> dpre1, in place
				}
		}
		__syncthreads();
		if (sums) coop_store(rs.dp1 + (size_t)row0 * rs.ldh + h * F, rs.ldh, F, Hs, rows, lane);
		for (int k0 = 0; k0 < Kd; k0 += HEADS_NJ) {
			dot_cols(w1, F, Kd, k0, Hs + lane, acc, lane);
#pragma unroll
			for (int kk = 0; kk < HEADS_NJ; kk++)
				if (k0 + kk < Kd) {
					float* p = &dXs[(k0 + kk) * HEADS_P + lane];
					*p = first ? acc[kk] : *p + acc[kk];
				}
		}
		__syncthreads();   // (Hs and Ds are the next head's)
		first = false;
	}
	if (first)
		for (int k = 0; k < Kd; k++) dXs[k * HEADS_P + lane] = 0.0f;
	__syncthreads();
	if (d_feat) coop_store(d_feat + (size_t)row0 * F, (size_t)F, F, dXs, rows, lane);
	if (d_anchor && valid) {
		const float vx = Xs[(F + 0) * HEADS_P + lane], vy = Xs[(F + 1) * HEADS_P + lane], vz = Xs[(F + 2) * HEADS_P + lane];
		const float dist = Xs[(F + 3) * HEADS_P + lane];
		const float gx = dXs[(F + 0) * HEADS_P + lane], gy = dXs[(F + 1) * HEADS_P + lane], gz = dXs[(F + 2) * HEADS_P + lane];
		const float gd = dXs[(F + 3) * HEADS_P + lane];
		const float s = (gx * vx + gy * vy) + gz * vz;
		float* p = d_anchor + (size_t)row * 3;
		p[0] = (gx - vx * s) / dist + gd * vx;
		p[1] = (gy - vy * s) / dist + gd * vy;
		p[2] = (gz - vz * s) / dist + gd * vz;
	}
}

// the checks both entry points share; fills the arguments
static int heads_args(const char* who, int n, int F, int K, const float* feat, long long fs, const float* anchor,
                      const float* cam, const float* mask, const bsr_heads_weights* w, HeadsArgs& a)
{
	if (n < 0) return fail("%s: n must be >= 0 (got %d)", who, n);
	if (F < 1 || F > BSR_HEADS_MAX_F) return fail("%s: F must be in [1, %d] (got %d)", who, BSR_HEADS_MAX_F, F);
	if (K < 1 || K > BSR_HEADS_MAX_K) return fail("%s: K must be in [1, %d] (got %d)", who, BSR_HEADS_MAX_K, K);
	if (!heads_shape_ok(n, F, K)) return fail("%s: n * max(7 K, F + 4) must be below 2^31 (got n = %d, F = %d, K = %d)", who, n, F, K);
	if (fs < F) return fail("%s: feat_stride must be >= F = %d (got %lld)", who, F, fs);
	if (!w) return fail("%s: NULL weights", who);
	uintptr_t bits = (uintptr_t)feat | (uintptr_t)anchor | (uintptr_t)cam | (uintptr_t)mask;
	for (int h = 0; h < 3; h++) {
		if (!w->head[h].w1 || !w->head[h].b1 || !w->head[h].w2 || !w->head[h].b2) return fail("%s: NULL weight tensor of head %d", who, h);
		bits |= (uintptr_t)w->head[h].w1 | (uintptr_t)w->head[h].b1 | (uintptr_t)w->head[h].w2 | (uintptr_t)w->head[h].b2;
	}
	if (n > 0 && (!feat || !anchor || !cam)) return fail("%s: NULL operand", who);
	if (bits & 3) return fail("%s: operands must be 4-byte aligned", who);
	a.n = n; a.F = F; a.K = K;
	a.feat = feat; a.fs = fs;
	a.anchor = anchor; a.cam = cam; a.mask = mask;
	a.w = *w;
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_anchor_heads_scratch_bytes(int n, int F, int K)
{
	if (!heads_shape_ok(n, F, K)) return 0;
	return align_up(heads_layout(n, F, K).floats * sizeof(float), 256);
}

int bsr_anchor_heads_forward(int n, int F, int K, const float* feat, long long feat_stride, const float* anchor,
                             const float* camera_center, const float* offset_mask, const bsr_heads_weights* w,
                             float* neural_opacity, float* color, float* scale_rot, float* maps, void* stream)
{
	const char* who = "bsr_anchor_heads_forward";
	HeadsArgs a;
	if (heads_args(who, n, F, K, feat, feat_stride, anchor, camera_center, offset_mask, w, a)) return 1;
	if (n == 0) return 0;
	if (!neural_opacity || !color || !scale_rot) return fail("%s: NULL output", who);
	if (((uintptr_t)neural_opacity | (uintptr_t)color | (uintptr_t)scale_rot | (uintptr_t)maps) & 3)
		return fail("%s: outputs must be 4-byte aligned", who);
	const size_t lds = (size_t)(2 * F + 4) * HEADS_P * sizeof(float);
	if (reserve_lds<k_heads_fwd>(who, lds)) return 1;
	const unsigned blocks = (unsigned)(((long long)n + HEADS_T - 1) / HEADS_T);
	hipLaunchKernelGGL(k_heads_fwd, dim3(blocks), dim3(HEADS_T), lds, (hipStream_t)stream, a, neural_opacity, color, scale_rot, maps);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_anchor_heads_backward(int n, int F, int K, const float* feat, long long feat_stride, const float* anchor,
                              const float* camera_center, const float* offset_mask, const bsr_heads_weights* w,
                              const float* color, const float* g_opacity, const float* g_color, const float* g_scale_rot,
                              float* d_feat, float* d_anchor, float* d_offset_mask, const bsr_heads_weight_grads* dw,
                              void* scratch, void* stream)
{
	const char* who = "bsr_anchor_heads_backward";
	HeadsArgs a;
	if (heads_args(who, n, F, K, feat, feat_stride, anchor, camera_center, offset_mask, w, a)) return 1;
	if (d_offset_mask && !offset_mask) return fail("%s: d_offset_mask without an offset_mask", who);
	if (((uintptr_t)color | (uintptr_t)g_opacity | (uintptr_t)g_color | (uintptr_t)g_scale_rot | (uintptr_t)d_feat |
	     (uintptr_t)d_anchor | (uintptr_t)d_offset_mask) & 3)
		return fail("%s: upstreams and gradients must be 4-byte aligned", who);
	const MlpSegments grads = heads_segments(F, K, dw);
	if (mlp_wgrad_check(who, grads)) return 1;
	const bool sums = mlp_wgrad_asked(grads);
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) return mlp_wgrad_zero(who, grads, st);
	if (g_color && !color) return fail("%s: g_color needs the forward's color", who);
	const MlpWgradLayout l = heads_layout(n, F, K);
	MlpRowScratch rs;
	if (mlp_wgrad_carve(who, l, sums, scratch, rs)) return 1;
	const size_t lds = (size_t)(3 * F + 8 + 7 * K) * HEADS_P * sizeof(float);
	if (reserve_lds<k_heads_bwd_rows>(who, lds)) return 1;
	const unsigned blocks = (unsigned)(((long long)n + HEADS_T - 1) / HEADS_T);
	hipLaunchKernelGGL(k_heads_bwd_rows, dim3(blocks), dim3(HEADS_T), lds, st, a, color, g_opacity, g_color, g_scale_rot, d_feat,
	                   d_anchor, d_offset_mask, rs);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	if (!sums) return 0;
	return mlp_wgrad_sums(who, heads_products(F, K, rs, grads), grads, n, l, scratch, st);
}

}  // extern "C"
