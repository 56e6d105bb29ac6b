// The context model's head of generate_neural_gaussians for gfx950 (include/bloomscene_context.h): mlp_grid on the
// hash-grid encoding of the visible anchors, the three adaptive step sizes, and either the noise injection of training
// or the STE_multistep quantiser of rendering.
//
//   k_context_fwd        enc -> hid -> pre2 = context, Q, the noised attributes
//   k_context_quantise   enc -> hid -> the last three rows of layer 2 -> Q -> the quantised attributes
//   k_context_bwd_rows   recomputes hid and the adjustments, forms dpre2 / dpre1 / d enc per row; with a weight gradient
//                        asked for it also leaves enc, hid, dpre1, dpre2 of every row in the scratch
//   k_mlp_wgrad, k_mlp_wsum (mlp_wgrad.h)   the weight gradients from that scratch: context_segments, context_products
//
// The lane mapping and the products are those of mlp_rows.h (a lane per row, 64 rows per workgroup, [index][lane] planes
// in LDS, 8 x 8 weights per vector load); unlike the heads' one wave, a workgroup here is several waves that share the
// rows' planes and split the blocks of eight outputs among them (CTX_FWD_WAVES, CTX_BWD_WAVES below).  pre2 blocks are
// stored straight from the accumulators, so the forward holds enc and hid only; the three adjustment columns are picked
// out of their blocks on the way.  The elementwise tails run
// cooperatively (consecutive lanes on consecutive elements of a row) with the row's Q read from LDS.  The row pass holds
// enc, hid and one plane per column of dpre2 -- 129 KB at the limits -- and reuses the planes: g_out / noise are staged
// in dpre2's before g_context is, hid turns into dpre1 in place, and d enc is formed in enc's.
#include "common.h"
#include "lds_reserve.h"
#include "mlp_rows.h"
#include "mlp_wgrad.h"
#include "../../include/bloomscene_context.h"

namespace bsr {

#define CTX_T MLP_ROWS_T
#define CTX_P MLP_ROWS_P
#define CTX_NJ MLP_ROWS_NJ
// Waves of a workgroup.  They share the 64 rows and their planes in LDS and split the blocks of eight outputs of every
// product among them: LDS, not registers, limits how many workgroups a CU holds (one of the row pass at BloomScene's
// shape), and a lone wave per SIMD cannot hide its own LDS and weight-load latencies.
#define CTX_FWD_WAVES 4
#define CTX_BWD_WAVES 8
#define CTX_MAX_THREADS 512

struct ContextArgs {
	int n, D, H, F, K, O;
	const float* enc;
	long long es;
	bsr_context_weights w;
	float q[3];
};

// the three attributes (feat, grid_scaling, grid_offsets) of a tail: x through a row stride, a dense second operand
// (the noise; unused by the quantiser), a dense output.  x == NULL: the attribute is left out.
struct ContextTail {
	const float* x[3];
	long long xs[3];
	const float* noise[3];
	float* out[3];
	const float* mean[3];
};

static int context_outputs(int F, int K) { return 2 * F + 12 + 6 * K + 3; }

// Element order of a partial: W1 [H, D], b1 [H], W2 [O, H], b2 [O].
static MlpSegments context_segments(int D, int H, int O, const bsr_context_weight_grads* dw)
{
	const bsr_context_weight_grads g = dw ? *dw : bsr_context_weight_grads{};
	MlpSegments d = {};
	d.add(H * D, g.w1);
	d.add(H, g.b1);
	d.add(O * H, g.w2);
	d.add(O, g.b2);
	return d;
}

static MlpProducts context_products(int D, int H, int O, const MlpRowScratch& rs, const MlpSegments& d)
{
	MlpProducts p = {};
	p.add(rs.dp1, rs.ldh, rs.x, rs.ldx, H, D, d, 0, 1);
	p.add(rs.dp2, rs.ld2, rs.hid, rs.ldh, O, H, d, 2, 3);
	return p;
}

// enc [D], hid / dp1 [H], dp2 [O]
static MlpWgradLayout context_layout(int n, int D, int H, int F, int K)
{
	const int O = context_outputs(F, K);
	return mlp_wgrad_layout(n, D, H, O, context_segments(D, H, O, nullptr).tot);
}

static bool context_shape_ok(int n, int D, int H, int F, int K)
{
	if (n < 0 || D < 1 || D > BSR_CONTEXT_MAX_D || H < 1 || H > BSR_CONTEXT_MAX_H) return false;
	if (F < 1 || F > BSR_CONTEXT_MAX_F || K < 1 || K > BSR_CONTEXT_MAX_K) return false;
	const long long O = context_outputs(F, K), widest = O > D ? O : D;
	return (long long)n * widest < (1LL << 31);
}

__device__ __forceinline__ int context_width(int c, int F, int K) { return c == 0 ? F : (c == 1 ? 6 : 3 * K); }

// The threads of a workgroup: `lane` is the row, `wave` (uniform over the wave) takes every `waves`-th block of eight
// outputs of a product, `tid` / `threads` walk the cooperative loads and stores.
struct ContextThread {
	int tid, threads, lane, wave, waves;
};

__device__ __forceinline__ ContextThread context_thread()
{
	ContextThread t;
	t.tid = threadIdx.x;
	t.threads = blockDim.x;
	t.lane = t.tid & (CTX_T - 1);
	t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
	t.waves = t.threads >> 6;
	return t;
}

// enc of the workgroup's rows -> Xs [D][lane]; rows past n are zeros
__device__ __forceinline__ void stage_enc(const ContextArgs& a, float* Xs, long long row0, int rows, const ContextThread& t)
{
	const int D = a.D;
	for (int idx = t.tid; idx < CTX_T * D; idx += t.threads) {
		const int r = idx / D, k = idx - r * D;
		Xs[k * CTX_P + r] = r < rows ? a.enc[(row0 + r) * a.es + k] : 0.0f;
	}
}

// Hs = relu(pre1) of the lane's row, this wave's blocks of it; pre1 (the lane's row of the map, or NULL) is written on the way
__device__ __forceinline__ void hidden_layer(const ContextArgs& a, const float* Xs, float* Hs, float* pre1, const ContextThread& t)
{
	float acc[CTX_NJ];
	for (int j0 = t.wave * CTX_NJ; j0 < a.H; j0 += t.waves * CTX_NJ) {
		chain_rows(a.w.w1, a.w.b1, a.H, a.D, j0, Xs + t.lane, acc, t.lane);
#pragma unroll
		for (int jj = 0; jj < CTX_NJ; jj++)
			if (j0 + jj < a.H) {
				if (pre1) pre1[j0 + jj] = acc[jj];
				Hs[(j0 + jj) * CTX_P + t.lane] = mlp_relu(acc[jj]);
			}
	}
}

// adj = pre2[O - 3 .. O - 1] alone: the block of layer 2 that starts at row O - 3 (its other five accumulators repeat the
// last row).  The chain of an output does not depend on the block it is evaluated in: the bits of the full layer.
__device__ __forceinline__ void adjustments(const ContextArgs& a, const float* Hs, float* adj, int lane)
{
	float acc[CTX_NJ];
	chain_rows(a.w.w2, a.w.b2, a.O, a.H, a.O - 3, Hs + lane, acc, lane);
	adj[0] = acc[0];
	adj[1] = acc[1];
	adj[2] = acc[2];
}

__device__ __forceinline__ float step_size(float q, float adj) { return q * (1.0f + mlp_tanh(adj)); }

__global__ void __launch_bounds__(CTX_MAX_THREADS) k_context_fwd(ContextArgs a, ContextTail t, float* __restrict__ context,
                                                                 float* __restrict__ Q, float* __restrict__ maps)
{
	extern __shared__ float ctx_lds[];
	const ContextThread th = context_thread();
	const int D = a.D, H = a.H, O = a.O, lane = th.lane;
	float* Xs = ctx_lds;
	float* Hs = Xs + D * CTX_P;
	float* Qs = Hs + H * CTX_P;   // [3][lane]
	const long long row0 = (long long)blockIdx.x * CTX_T, row = row0 + lane;
	const long long left = (long long)a.n - row0;
	const int rows = left < CTX_T ? (int)left : CTX_T;
	const bool valid = lane < rows;
	stage_enc(a, Xs, row0, rows, th);
	__syncthreads();
	hidden_layer(a, Xs, Hs, maps && valid ? maps + (size_t)row * H : nullptr, th);
	__syncthreads();
	float acc[CTX_NJ];
	float* out = context + (size_t)row * O;
	for (int o0 = th.wave * CTX_NJ; o0 < O; o0 += th.waves * CTX_NJ) {
		chain_rows(a.w.w2, a.w.b2, O, H, o0, Hs + lane, acc, lane);
		const int first = O - 3 - o0;   // (uniform) where the adjustment columns start in this block
		if (first > -3 && first < CTX_NJ) {
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const int at = first + c;
				if (at < 0 || at >= CTX_NJ) continue;
				float adj = acc[0];
#pragma unroll
				for (int jj = 1; jj < CTX_NJ; jj++) adj = jj == at ? acc[jj] : adj;
				const float s = step_size(a.q[c], adj);   // its step size, from the wave that holds the column
				if (valid) Q[(size_t)row * 3 + c] = s;
				Qs[c * CTX_P + lane] = s;
			}
		}
		if (valid) store_block(out + o0, acc, O - o0);
	}
	__syncthreads();
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (!t.x[c]) continue;
		const int C = context_width(c, a.F, a.K);
		const float* noise = t.noise[c] + (size_t)row0 * C;
		float* dst = t.out[c] + (size_t)row0 * C;
		for (int idx = th.tid; idx < rows * C; idx += th.threads) {
			const int r = idx / C, k = idx - r * C;
			const float sigma = Qs[c * CTX_P + r] + 1e-6f;                       // GR:87-89
			dst[idx] = t.x[c][(row0 + r) * t.xs[c] + k] + noise[idx] * sigma;     // GR:91-97
		}
	}
}

__global__ void __launch_bounds__(CTX_MAX_THREADS) k_context_quantise(ContextArgs a, ContextTail t, float* __restrict__ Q)
{
	extern __shared__ float ctx_lds[];
	const ContextThread th = context_thread();
	const int D = a.D, H = a.H, lane = th.lane;
	float* Xs = ctx_lds;
	float* Hs = Xs + D * CTX_P;
	float* Qs = Hs + H * CTX_P;
	const long long row0 = (long long)blockIdx.x * CTX_T, row = row0 + lane;
	const long long left = (long long)a.n - row0;
	const int rows = left < CTX_T ? (int)left : CTX_T;
	const bool valid = lane < rows;
	stage_enc(a, Xs, row0, rows, th);
	__syncthreads();
	hidden_layer(a, Xs, Hs, nullptr, th);
	__syncthreads();
	if (th.wave == 0) {   // (one block of layer 2: one wave's work)
		float adj[3];
		adjustments(a, Hs, adj, lane);
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const float s = step_size(a.q[c], adj[c]);
			if (Q && valid) Q[(size_t)row * 3 + c] = s;
			Qs[c * CTX_P + lane] = s;
		}
	}
	__syncthreads();
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (!t.x[c]) continue;
		const int C = context_width(c, a.F, a.K);
		const float m = uload(t.mean[c], 0);
		float* dst = t.out[c] + (size_t)row0 * C;
		for (int idx = th.tid; idx < rows * C; idx += th.threads) {
			const int r = idx / C, k = idx - r * C;
			const float q = Qs[c * CTX_P + r];
			const float lo = m - 15000.0f * q, hi = m + 15000.0f * q;
			float x = t.x[c][(row0 + r) * t.xs[c] + k];
			x = x < lo ? lo : x;
			x = x > hi ? hi : x;
			const float qq = rintf(x / q) * q;
			dst[idx] = qq + mlp_tanh(x - qq) * q;
		}
	}
}

struct ContextUpstreams {
	const float *g_context, *g_q;
	const float* g_out[3];
	const float* noise[3];
};

__global__ void __launch_bounds__(CTX_MAX_THREADS) k_context_bwd_rows(ContextArgs a, ContextUpstreams u, float* __restrict__ d_enc,
                                                                      MlpRowScratch rs)
{
	extern __shared__ float ctx_lds[];
	const ContextThread th = context_thread();
	const int D = a.D, H = a.H, O = a.O, lane = th.lane;
	float* Xs = ctx_lds;
	float* Hs = Xs + D * CTX_P;
	float* Ds = Hs + H * CTX_P;   // [O][lane]
	const long long row0 = (long long)blockIdx.x * CTX_T, row = row0 + lane;
	const long long left = (long long)a.n - row0;
	const int rows = left < CTX_T ? (int)left : CTX_T;
	const bool valid = lane < rows;
	const bool sums = rs.x != nullptr;
	stage_enc(a, Xs, row0, rows, th);
	__syncthreads();
	if (sums) coop_store(rs.x + (size_t)row0 * rs.ldx, rs.ldx, D, Xs, rows, th.tid, th.threads);
	hidden_layer(a, Xs, Hs, nullptr, th);
	__syncthreads();
	if (sums) coop_store(rs.hid + (size_t)row0 * rs.ldh, rs.ldh, H, Hs, rows, th.tid, th.threads);
	// dadj: only with an upstream that reaches Q.  The chains over a row's g_out and its three adjustments are wave 0's.
	const bool through_q = u.g_q || u.g_out[0] || u.g_out[1] || u.g_out[2];
	float dadj[3] = {0.0f, 0.0f, 0.0f};
	if (through_q) {
		float dq[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			dq[c] = u.g_q && valid ? u.g_q[(size_t)row * 3 + c] : 0.0f;
			if (!u.g_out[c]) continue;
			const int C = context_width(c, a.F, a.K);   // (2 C <= O planes: g_out in the first C, the noise behind it)
			const size_t at = (size_t)row0 * C;
			for (int idx = th.tid; idx < CTX_T * C; idx += th.threads) {
				const int r = idx / C, k = idx - r * C;
				Ds[k * CTX_P + r] = r < rows ? u.g_out[c][at + idx] : 0.0f;
				Ds[(C + k) * CTX_P + r] = r < rows ? u.noise[c][at + idx] : 0.0f;
			}
			__syncthreads();
			if (th.wave == 0)
				for (int k = 0; k < C; k++) dq[c] = fmaf(Ds[k * CTX_P + lane], Ds[(C + k) * CTX_P + lane], dq[c]);
			__syncthreads();
		}
		if (th.wave == 0) {
			float adj[3];
			adjustments(a, Hs, adj, lane);
#pragma unroll
			for (int c = 0; c < 3; c++) {
				const float tn = mlp_tanh(adj[c]);
				dadj[c] = (dq[c] * a.q[c]) * (1.0f - tn * tn);
			}
		}
	}
	for (int idx = th.tid; idx < CTX_T * O; idx += th.threads) {
		const int r = idx / O, o = idx - r * O;
		Ds[o * CTX_P + r] = u.g_context && r < rows ? u.g_context[(size_t)row0 * O + idx] : 0.0f;
	}
	__syncthreads();
	if (through_q && th.wave == 0 && valid) {
#pragma unroll
		for (int c = 0; c < 3; c++) Ds[(O - 3 + c) * CTX_P + lane] = Ds[(O - 3 + c) * CTX_P + lane] + dadj[c];
	}
	__syncthreads();
	if (sums) coop_store(rs.dp2 + (size_t)row0 * rs.ld2, rs.ld2, O, Ds, rows, th.tid, th.threads);
	float acc[CTX_NJ];
	for (int j0 = th.wave * CTX_NJ; j0 < H; j0 += th.waves * CTX_NJ) {
		dot_cols(a.w.w2, O, H, j0, Ds + lane, acc, lane);
#pragma unroll
		for (int jj = 0; jj < CTX_NJ; jj++)
			if (j0 + jj < H) {
				float* p = &Hs[(j0 + jj) * CTX_P + lane];
				*p = *p > 0.0f ? acc[jj] : 0.0f;   // hid -> dpre1, in place (an element is read and written by one wave)
			}
	}
	__syncthreads();
	if (sums) coop_store(rs.dp1 + (size_t)row0 * rs.ldh, rs.ldh, H, Hs, rows, th.tid, th.threads);
	if (!d_enc) return;
	for (int k0 = th.wave * CTX_NJ; k0 < D; k0 += th.waves * CTX_NJ) {   // (enc is not read any more: d enc takes its planes)
		dot_cols(a.w.w1, H, D, k0, Hs + lane, acc, lane);
#pragma unroll
		for (int kk = 0; kk < CTX_NJ; kk++)
			if (k0 + kk < D) Xs[(k0 + kk) * CTX_P + lane] = acc[kk];
	}
	__syncthreads();
	coop_store(d_enc + (size_t)row0 * D, (size_t)D, D, Xs, rows, th.tid, th.threads);
}

// the checks the entry points share; fills the arguments
static int context_args(const char* who, int n, int D, int H, int F, int K, const float* enc, long long es,
                        const bsr_context_weights* w, float qf, float qs, float qo, ContextArgs& a)
{
	if (n < 0) return fail("%s: n must be >= 0 (got %d)", who, n);
	if (D < 1 || D > BSR_CONTEXT_MAX_D) return fail("%s: D must be in [1, %d] (got %d)", who, BSR_CONTEXT_MAX_D, D);
	if (H < 1 || H > BSR_CONTEXT_MAX_H) return fail("%s: H must be in [1, %d] (got %d)", who, BSR_CONTEXT_MAX_H, H);
	if (F < 1 || F > BSR_CONTEXT_MAX_F) return fail("%s: F must be in [1, %d] (got %d)", who, BSR_CONTEXT_MAX_F, F);
	if (K < 1 || K > BSR_CONTEXT_MAX_K) return fail("%s: K must be in [1, %d] (got %d)", who, BSR_CONTEXT_MAX_K, K);
	if (!context_shape_ok(n, D, H, F, K))
		return fail("%s: n * max(2 F + 12 + 6 K + 3, D) must be below 2^31 (got n = %d, D = %d, F = %d, K = %d)", who, n, D, F, K);
	if (es < D) return fail("%s: enc_stride must be >= D = %d (got %lld)", who, D, es);
	if (!w) return fail("%s: NULL weights", who);
	if (!w->w1 || !w->b1 || !w->w2 || !w->b2) return fail("%s: NULL weight tensor", who);
	if (n > 0 && !enc) return fail("%s: NULL enc", who);
	if (((uintptr_t)enc | (uintptr_t)w->w1 | (uintptr_t)w->b1 | (uintptr_t)w->w2 | (uintptr_t)w->b2) & 3)
		return fail("%s: operands must be 4-byte aligned", who);
	a.n = n; a.D = D; a.H = H; a.F = F; a.K = K; a.O = context_outputs(F, K);
	a.enc = enc; a.es = es;
	a.w = *w;
	a.q[0] = qf; a.q[1] = qs; a.q[2] = qo;
	return 0;
}

// one attribute of a tail: all of its pointers or none, the stride wide enough, everything 4-byte aligned
static int context_attribute(const char* who, const char* name, int C, const float* x, long long xs, const float* second,
                             const char* second_name, const float* out)
{
	if (!x) {
		if (second || out) return fail("%s: %s is NULL but its %s or output is not", who, name, second_name);
		return 0;
	}
	if (!second) return fail("%s: %s without its %s", who, name, second_name);
	if (!out) return fail("%s: %s without its output", who, name);
	if (xs < C) return fail("%s: %s_stride must be >= %d (got %lld)", who, name, C, xs);
	if (((uintptr_t)x | (uintptr_t)second | (uintptr_t)out) & 3) return fail("%s: %s operands must be 4-byte aligned", who, name);
	return 0;
}

static unsigned context_blocks(int n) { return (unsigned)(((long long)n + CTX_T - 1) / CTX_T); }

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_context_scratch_bytes(int n, int D, int H, int F, int K)
{
	if (!context_shape_ok(n, D, H, F, K)) return 0;
	return align_up(context_layout(n, D, H, F, K).floats * sizeof(float), 256);
}

int bsr_context_head_forward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                             const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                             const float* feat, long long feat_stride, const float* scaling, long long scaling_stride,
                             const float* offsets, long long offsets_stride, const float* noise_feat,
                             const float* noise_scaling, const float* noise_offsets, float* context, float* Q,
                             float* out_feat, float* out_scaling, float* out_offsets, float* maps, void* stream)
{
	const char* who = "bsr_context_head_forward";
	ContextArgs a;
	if (context_args(who, n, D, H, F, K, enc, enc_stride, w, q_feat, q_scaling, q_offsets, a)) return 1;
	if (context_attribute(who, "feat", F, feat, feat_stride, noise_feat, "noise", out_feat)) return 1;
	if (context_attribute(who, "scaling", 6, scaling, scaling_stride, noise_scaling, "noise", out_scaling)) return 1;
	if (context_attribute(who, "offsets", 3 * K, offsets, offsets_stride, noise_offsets, "noise", out_offsets)) return 1;
	if (n == 0) return 0;
	if (!context || !Q) return fail("%s: NULL output", who);
	if (((uintptr_t)context | (uintptr_t)Q | (uintptr_t)maps) & 3) return fail("%s: outputs must be 4-byte aligned", who);
	ContextTail t = {{feat, scaling, offsets}, {feat_stride, scaling_stride, offsets_stride},
	                 {noise_feat, noise_scaling, noise_offsets}, {out_feat, out_scaling, out_offsets}, {nullptr, nullptr, nullptr}};
	const size_t lds = (size_t)(D + H + 3) * CTX_P * sizeof(float);
	if (reserve_lds<k_context_fwd>(who, lds)) return 1;
	hipLaunchKernelGGL(k_context_fwd, dim3(context_blocks(n)), dim3(CTX_T * CTX_FWD_WAVES), lds, (hipStream_t)stream, a, t, context, Q, maps);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_context_quantise_forward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                                 const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                                 const float* feat, long long feat_stride, const float* scaling, long long scaling_stride,
                                 const float* offsets, long long offsets_stride, const float* feat_mean,
                                 const float* scaling_mean, const float* offsets_mean, float* Q, float* out_feat,
                                 float* out_scaling, float* out_offsets, void* stream)
{
	const char* who = "bsr_context_quantise_forward";
	ContextArgs a;
	if (context_args(who, n, D, H, F, K, enc, enc_stride, w, q_feat, q_scaling, q_offsets, a)) return 1;
	if (context_attribute(who, "feat", F, feat, feat_stride, feat_mean, "mean", out_feat)) return 1;
	if (context_attribute(who, "scaling", 6, scaling, scaling_stride, scaling_mean, "mean", out_scaling)) return 1;
	if (context_attribute(who, "offsets", 3 * K, offsets, offsets_stride, offsets_mean, "mean", out_offsets)) return 1;
	if (n == 0) return 0;
	if ((uintptr_t)Q & 3) return fail("%s: Q must be 4-byte aligned", who);
	ContextTail t = {{feat, scaling, offsets}, {feat_stride, scaling_stride, offsets_stride}, {nullptr, nullptr, nullptr},
	                 {out_feat, out_scaling, out_offsets}, {feat_mean, scaling_mean, offsets_mean}};
	const size_t lds = (size_t)(D + H + 3) * CTX_P * sizeof(float);
	if (reserve_lds<k_context_quantise>(who, lds)) return 1;
	hipLaunchKernelGGL(k_context_quantise, dim3(context_blocks(n)), dim3(CTX_T * CTX_FWD_WAVES), lds, (hipStream_t)stream, a, t, Q);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_context_head_backward(int n, int D, int H, int F, int K, const float* enc, long long enc_stride,
                              const bsr_context_weights* w, float q_feat, float q_scaling, float q_offsets,
                              const float* noise_feat, const float* noise_scaling, const float* noise_offsets,
                              const float* g_context, const float* g_Q, const float* g_out_feat,
                              const float* g_out_scaling, const float* g_out_offsets, float* d_enc,
                              const bsr_context_weight_grads* dw, void* scratch, void* stream)
{
	const char* who = "bsr_context_head_backward";
	ContextArgs a;
	if (context_args(who, n, D, H, F, K, enc, enc_stride, w, q_feat, q_scaling, q_offsets, a)) return 1;
	ContextUpstreams u = {g_context, g_Q, {g_out_feat, g_out_scaling, g_out_offsets}, {noise_feat, noise_scaling, noise_offsets}};
	static const char* const names[3] = {"feat", "scaling", "offsets"};
	uintptr_t bits = (uintptr_t)g_context | (uintptr_t)g_Q | (uintptr_t)d_enc;
	for (int c = 0; c < 3; c++) {
		if (u.g_out[c] && !u.noise[c]) return fail("%s: g_out_%s needs the forward's noise_%s", who, names[c], names[c]);
		bits |= (uintptr_t)u.g_out[c] | (uintptr_t)u.noise[c];
	}
	if (bits & 3) return fail("%s: upstreams and gradients must be 4-byte aligned", who);
	const MlpSegments grads = context_segments(D, H, a.O, dw);
	if (mlp_wgrad_check(who, grads)) return 1;
	const bool sums = mlp_wgrad_asked(grads);
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) return mlp_wgrad_zero(who, grads, st);
	const MlpWgradLayout l = context_layout(n, D, H, F, K);
	MlpRowScratch rs;
	if (mlp_wgrad_carve(who, l, sums, scratch, rs)) return 1;
	const size_t lds = ((size_t)D + H + a.O) * CTX_P * sizeof(float);
	if (reserve_lds<k_context_bwd_rows>(who, lds)) return 1;
	hipLaunchKernelGGL(k_context_bwd_rows, dim3(context_blocks(n)), dim3(CTX_T * CTX_BWD_WAVES), lds, st, a, u, d_enc, rs);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	if (!sums) return 0;
	return mlp_wgrad_sums(who, context_products(D, H, a.O, rs, grads), grads, n, l, scratch, st);
}

}  // extern "C"
