// The three anchor MLP heads of generate_neural_gaussians for gfx950 (include/bloomscene_heads.h): mlp_opacity, mlp_cov and
// mlp_color on the visible anchors, with the view geometry, the reshapes and the offset mask folded in.
//
//   k_heads_fwd        X -> hid -> pre2 -> the three outputs, one head after the other
//   k_heads_bwd_rows   recomputes hid, forms dpre2 / dpre1 / dX per row -> d feat, d anchor, d offset_mask; with a weight
//                      gradient asked for it also leaves X, hid, dpre1, dpre2 of every row in the scratch
//   k_heads_wgrad      per range of BSR_HEADS_CHUNK rows one partial of every weight-gradient element
//   k_heads_wsum       adds the partials of an element in ascending range order
//
// LANE MAPPING (forward and row pass).  A lane is an anchor row; a workgroup is ONE wave of 64 rows.  The row's vectors
// that are indexed by a loop variable (X, hid, dpre2, dX) live in LDS as [index][lane] with a pitch of 65 floats: the
// lane's own column is read without bank conflicts, and the cooperative, coalesced loads and stores of whole rows walk it
// with a stride of 65 (conflict-free as well).  Eight outputs are accumulated at a time in registers; their weights are
// uniform over the wave: a block of 8 x 8 of them is one coalesced vector load, and each FMA takes its weight from a lane
// of it as a scalar operand (mlp_rows.h, which holds these products: THE WEIGHTS OF A STEP), with one LDS read per eight
// FMAs.  Every chain is written with explicit fmaf in the order the header states: the build stays at -ffp-contract=off.
// WEIGHT GRADIENTS.  The reduction index is the row, which the row pass has on the lane; so that pass stores its per-row
// operands (row-major, rows padded to 16 bytes) and k_heads_wgrad runs dW = dpre^T X as a register-blocked product: a
// thread owns a 4 x 4 block of one weight matrix and walks its range of rows in order, two 16-byte loads per 16 FMAs
// (fp64 ones: the sums over rows are the one place where fp32 accumulation in a fixed order loses to a library's tree).
// The grid is a function of (n, F, K) alone.
#include <atomic>
#include "common.h"
#include "mlp_rows.h"   // uload, lane_value, step_fma, chain_rows, dot_cols, coop_store, store_block, the activations
#include "../../include/bloomscene_heads.h"

namespace bsr {

#define HEADS_T MLP_ROWS_T     // rows a workgroup (one wave)
#define HEADS_P MLP_ROWS_P     // LDS pitch of a [index][lane] vector
#define HEADS_NJ MLP_ROWS_NJ   // outputs accumulated at a time
#define HEADS_SUM_BLOCK 256

struct HeadsArgs {
	int n, F, K;
	const float* feat;
	long long fs;
	const float *anchor, *cam, *mask;
	bsr_heads_weights w;
};

// what the row pass leaves for the weight-gradient sums (all NULL: nothing is left)
struct HeadsRowScratch {
	float *x, *hid, *dp1, *dp2;
	size_t ldx, ldh, ld2;
};

struct HeadsLayout {
	size_t ldx, ldh, ld2;       // row pitches (floats) of x [F + 4], hid / dp1 [3 F], dp2 [11 K]: a multiple of 4, + 4
	size_t chunks;              // ranges of BSR_HEADS_CHUNK rows
	int tot;                    // weight-gradient elements: W1 (3 heads), b1, W2, b2
	size_t off_hid, off_dp1, off_dp2, off_partials, floats;
};

static HeadsLayout heads_layout(int n, int F, int K)
{
	HeadsLayout l;
	l.ldx = (((size_t)F + 4 + 3) & ~(size_t)3) + 4;
	l.ldh = ((3 * (size_t)F + 3) & ~(size_t)3) + 4;
	l.ld2 = ((11 * (size_t)K + 3) & ~(size_t)3) + 4;
	l.chunks = ((size_t)n + BSR_HEADS_CHUNK - 1) / BSR_HEADS_CHUNK;
	l.tot = 3 * F * (F + 4) + 3 * F + 11 * K * F + 11 * K;
	l.off_hid = (size_t)n * l.ldx;
	l.off_dp1 = l.off_hid + (size_t)n * l.ldh;
	l.off_dp2 = l.off_dp1 + (size_t)n * l.ldh;
	l.off_partials = l.off_dp2 + (size_t)n * l.ld2;
	l.floats = l.off_partials + l.chunks * (size_t)l.tot + 64;
	return l;
}

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

__device__ __forceinline__ void coop_zero(float* dst, size_t ld, int C, int rows, int lane)
{
	for (int idx = lane; idx < rows * C; idx += HEADS_T) {
		const int r = idx / C, c = idx - r * C;
		dst[(size_t)r * ld + c] = 0.0f;
	}
}

__device__ __forceinline__ int heads_outputs(int h, int K) { return h == 0 ? K : (h == 1 ? 7 * K : 3 * K); }
__device__ __forceinline__ int heads_offset(int h, int K) { return h == 0 ? 0 : (h == 1 ? K : 8 * K); }

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
					Hs[(j0 + jj) * HEADS_P + lane] = heads_relu(acc[jj]);
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
					const float t = heads_tanh(acc[jj]);
					acc[jj] = a.mask && jj < count ? t * a.mask[(size_t)row * K + o0 + jj] : t;
				}
			} else if (h == 2) {
#pragma unroll
				for (int jj = 0; jj < HEADS_NJ; jj++) acc[jj] = heads_sigmoid(acc[jj]);
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
                                                            HeadsRowScratch rs)
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
				if (j0 + jj < F) Hs[(j0 + jj) * HEADS_P + lane] = heads_relu(acc[jj]);
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
						const float t = heads_tanh(acc[jj]);
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

struct HeadsSumArgs {
	int n, F, K, tot;
	const float *x, *hid, *dp1, *dp2;
	size_t ldx, ldh, ld2;
	float* partials;
};

// Element order of a partial (and of k_heads_wsum): W1 of the three heads [3 F, F + 4], b1 [3 F], W2 [11 K, F], b2 [11 K].
__global__ void __launch_bounds__(HEADS_SUM_BLOCK) k_heads_wgrad(HeadsSumArgs s)
{
	const int F = s.F, K = s.K, Kd = F + 4;
	int u = blockIdx.y * HEADS_SUM_BLOCK + threadIdx.x;
	const int KB0 = (Kd + 3) >> 2, JB0 = (3 * F + 3) >> 2, KB = (F + 3) >> 2;
	const float *A, *B;
	size_t lda, ldb;
	int jv, kv, out, outld, bout, kb;
	if (u < JB0 * KB0) {
		const int jb = u / KB0;
		kb = u - jb * KB0;
		A = s.dp1 + 4 * jb; lda = s.ldh;
		B = s.x + 4 * kb; ldb = s.ldx;
		jv = 3 * F - 4 * jb; kv = Kd - 4 * kb;
		out = 4 * jb * Kd + 4 * kb; outld = Kd;
		bout = 3 * F * Kd + 4 * jb;
	} else {
		u -= JB0 * KB0;
		int h = 0, off = 0, O = K;
		for (; h < 3; h++) {
			O = heads_outputs(h, K);
			const int units = ((O + 3) >> 2) * KB;
			if (u < units) break;
			u -= units;
			off += O;
		}
		if (h == 3) return;
		const int jb = u / KB;
		kb = u - jb * KB;
		A = s.dp2 + off + 4 * jb; lda = s.ld2;
		B = s.hid + h * F + 4 * kb; ldb = s.ldh;
		jv = O - 4 * jb; kv = F - 4 * kb;
		out = 3 * F * Kd + 3 * F + (off + 4 * jb) * F + 4 * kb; outld = F;
		bout = 3 * F * Kd + 3 * F + 11 * K * F + off + 4 * jb;
	}
	const size_t r0 = (size_t)blockIdx.x * BSR_HEADS_CHUNK;
	const size_t r1 = r0 + BSR_HEADS_CHUNK < (size_t)s.n ? r0 + BSR_HEADS_CHUNK : (size_t)s.n;
	// fp64: a product of two fp32 values is exact there, so a range's sum is rounded once, when it is stored
	double acc[4][4], ab[4];
#pragma unroll
	for (int jj = 0; jj < 4; jj++) {
		ab[jj] = 0.0;
#pragma unroll
		for (int kk = 0; kk < 4; kk++) acc[jj][kk] = 0.0;
	}
	for (size_t r = r0; r < r1; r++) {
		const bsr_f32x4 av = *reinterpret_cast<const bsr_f32x4_a4*>(A + r * lda);
		const bsr_f32x4 bv = *reinterpret_cast<const bsr_f32x4_a4*>(B + r * ldb);
		const double aa[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
		const double bb[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
		for (int jj = 0; jj < 4; jj++) {
			ab[jj] = ab[jj] + aa[jj];
#pragma unroll
			for (int kk = 0; kk < 4; kk++) acc[jj][kk] = fma(aa[jj], bb[kk], acc[jj][kk]);
		}
	}
	float* P = s.partials + (size_t)blockIdx.x * s.tot;
#pragma unroll
	for (int jj = 0; jj < 4; jj++) {
		if (jj >= jv) continue;
#pragma unroll
		for (int kk = 0; kk < 4; kk++)
			if (kk < kv) P[out + jj * outld + kk] = (float)acc[jj][kk];
		if (kb == 0) P[bout + jj] = (float)ab[jj];
	}
}

__global__ void __launch_bounds__(HEADS_SUM_BLOCK) k_heads_wsum(const float* __restrict__ partials, size_t chunks, int tot, int F,
                                                                int K, bsr_heads_weight_grads dw)
{
	int t = blockIdx.x * HEADS_SUM_BLOCK + threadIdx.x;
	if (t >= tot) return;
	double sum = (double)partials[t];
	for (size_t c = 1; c < chunks; c++) sum = sum + (double)partials[c * (size_t)tot + t];
	const float s = (float)sum;
	const int Kd = F + 4;
	float* p;
	int local;
	if (t < 3 * F * Kd) {
		const int h = t / (F * Kd);
		local = t - h * F * Kd;
		p = dw.head[h].w1;
	} else if ((t -= 3 * F * Kd) < 3 * F) {
		const int h = t / F;
		local = t - h * F;
		p = dw.head[h].b1;
	} else if ((t -= 3 * F) < 11 * K * F) {
		const int h = t < K * F ? 0 : (t < 8 * K * F ? 1 : 2);
		local = t - heads_offset(h, K) * F;
		p = dw.head[h].w2;
	} else {
		t -= 11 * K * F;
		const int h = t < K ? 0 : (t < 8 * K ? 1 : 2);
		local = t - heads_offset(h, K);
		p = dw.head[h].b2;
	}
	if (p) p[local] = s;
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

// a workgroup's LDS beyond the default 64 KiB has to be asked for (F and K near their limits in the row pass): once per
// kernel and DEVICE, with the device's whole LDS, not per call.  Two host threads that meet here both ask, which is
// harmless: the state is atomic and both store the same answer.
#define HEADS_MAX_DEVICES 64
template <typename Kern>
static int heads_lds_limit(Kern kern, size_t bytes)
{
	static std::atomic<int> state[HEADS_MAX_DEVICES];   // (one array per kernel type) 0 not asked yet, 1 granted, -1 refused
	if (bytes <= 64 * 1024) return 0;
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 1;
	const bool tracked = dev < HEADS_MAX_DEVICES;
	int st = tracked ? state[dev].load(std::memory_order_relaxed) : 0;
	if (st == 0) {
		st = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess ? 1 : -1;
		if (tracked) state[dev].store(st, std::memory_order_relaxed);
	}
	return st < 0;
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
	if (heads_lds_limit(k_heads_fwd, lds)) return fail("%s: cannot reserve %zu bytes of LDS", who, lds);
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
	bsr_heads_weight_grads grads = {};
	bool sums = false;
	if (dw) {
		grads = *dw;
		for (int h = 0; h < 3; h++) {
			sums = sums || grads.head[h].w1 || grads.head[h].b1 || grads.head[h].w2 || grads.head[h].b2;
			if (((uintptr_t)grads.head[h].w1 | (uintptr_t)grads.head[h].b1 | (uintptr_t)grads.head[h].w2 | (uintptr_t)grads.head[h].b2) & 3)
				return fail("%s: weight gradients must be 4-byte aligned", who);
		}
	}
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) {
		for (int h = 0; h < 3 && sums; h++) {
			const size_t O = h == 0 ? K : (h == 1 ? 7 * K : 3 * K);
			float* p[4] = {grads.head[h].w1, grads.head[h].b1, grads.head[h].w2, grads.head[h].b2};
			const size_t count[4] = {(size_t)F * (F + 4), (size_t)F, O * F, O};
			for (int i = 0; i < 4; i++)
				if (p[i] && hipMemsetAsync(p[i], 0, count[i] * sizeof(float), st) != hipSuccess) return fail("%s: memset failed", who);
		}
		return 0;
	}
	if (g_color && !color) return fail("%s: g_color needs the forward's color", who);
	if (sums && !scratch) return fail("%s: the weight gradients need the scratch", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	const HeadsLayout l = heads_layout(n, F, K);
	HeadsRowScratch rs = {};
	float* base = (float*)scratch;
	if (sums) {
		rs.x = base; rs.hid = base + l.off_hid; rs.dp1 = base + l.off_dp1; rs.dp2 = base + l.off_dp2;
		rs.ldx = l.ldx; rs.ldh = l.ldh; rs.ld2 = l.ld2;
	}
	const size_t lds = (size_t)(3 * F + 8 + 7 * K) * HEADS_P * sizeof(float);
	if (heads_lds_limit(k_heads_bwd_rows, lds)) return fail("%s: cannot reserve %zu bytes of LDS", who, lds);
	const unsigned blocks = (unsigned)(((long long)n + HEADS_T - 1) / HEADS_T);
	hipLaunchKernelGGL(k_heads_bwd_rows, dim3(blocks), dim3(HEADS_T), lds, st, a, color, g_opacity, g_color, g_scale_rot, d_feat,
	                   d_anchor, d_offset_mask, rs);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	if (!sums) return 0;
	HeadsSumArgs s;
	s.n = n; s.F = F; s.K = K; s.tot = l.tot;
	s.x = rs.x; s.hid = rs.hid; s.dp1 = rs.dp1; s.dp2 = rs.dp2;
	s.ldx = l.ldx; s.ldh = l.ldh; s.ld2 = l.ld2;
	s.partials = base + l.off_partials;
	const int KB = (F + 3) / 4;
	const int units = ((3 * F + 3) / 4) * ((F + 4 + 3) / 4) + (((K + 3) / 4) + ((7 * K + 3) / 4) + ((3 * K + 3) / 4)) * KB;
	hipLaunchKernelGGL(k_heads_wgrad, dim3((unsigned)l.chunks, (unsigned)((units + HEADS_SUM_BLOCK - 1) / HEADS_SUM_BLOCK)),
	                   dim3(HEADS_SUM_BLOCK), 0, st, s);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	hipLaunchKernelGGL(k_heads_wsum, dim3((unsigned)((l.tot + HEADS_SUM_BLOCK - 1) / HEADS_SUM_BLOCK)), dim3(HEADS_SUM_BLOCK), 0, st,
	                   s.partials, l.chunks, l.tot, F, K, grads);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
