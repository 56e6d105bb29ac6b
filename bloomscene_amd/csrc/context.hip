// The context model's head of generate_neural_gaussians for gfx950 (include/bloomscene_context.h): mlp_grid on the
// hash-grid encoding of the visible anchors, the three adaptive step sizes, and either the noise injection of training
// or the STE_multistep quantiser of rendering.
//
//   k_context_fwd        enc -> hid -> pre2 = context, Q, the noised attributes
//   k_context_quantise   enc -> hid -> the last three rows of layer 2 -> Q -> the quantised attributes
//   k_context_bwd_rows   recomputes hid and the adjustments, forms dpre2 / dpre1 / d enc per row; with a weight gradient
//                        asked for it also leaves enc, hid, dpre1, dpre2 of every row in the scratch
//   k_context_wgrad      per range of BSR_CONTEXT_CHUNK rows one partial of every weight-gradient element
//   k_context_wsum       adds the partials of an element in ascending range order
//
// The lane mapping and the products are those of mlp_rows.h (a lane per row, 64 rows per workgroup, [index][lane] planes
// in LDS, 8 x 8 weights per vector load); unlike the heads' one wave, a workgroup here is several waves that share the
// rows' planes and split the blocks of eight outputs among them (CTX_FWD_WAVES, CTX_BWD_WAVES below).  pre2 blocks are
// stored straight from the accumulators, so the forward holds enc and hid only; the three adjustment columns are picked
// out of their blocks on the way.  The elementwise tails run
// cooperatively (consecutive lanes on consecutive elements of a row) with the row's Q read from LDS.  The row pass holds
// enc, hid and one plane per column of dpre2 -- 129 KB at the limits -- and reuses the planes: g_out / noise are staged
// in dpre2's before g_context is, hid turns into dpre1 in place, and d enc is formed in enc's.  The weight-gradient sums
// are k_heads_wgrad's scheme for one stack.
#include <atomic>
#include "common.h"
#include "mlp_rows.h"
#include "../../include/bloomscene_context.h"

namespace bsr {

#define CTX_T MLP_ROWS_T
#define CTX_P MLP_ROWS_P
#define CTX_NJ MLP_ROWS_NJ
#define CTX_SUM_BLOCK 256
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

struct ContextRowScratch {
	float *x, *hid, *dp1, *dp2;
	size_t ldx, ldh, ld2;
};

struct ContextLayout {
	size_t ldx, ldh, ld2;       // row pitches (floats) of enc [D], hid / dp1 [H], dp2 [O]: a multiple of 4, + 4
	size_t chunks;              // ranges of BSR_CONTEXT_CHUNK rows
	int tot;                    // weight-gradient elements: W1, b1, W2, b2
	size_t off_hid, off_dp1, off_dp2, off_partials, floats;
};

static int context_outputs(int F, int K) { return 2 * F + 12 + 6 * K + 3; }

static ContextLayout context_layout(int n, int D, int H, int F, int K)
{
	const size_t O = (size_t)context_outputs(F, K);
	ContextLayout l;
	l.ldx = (((size_t)D + 3) & ~(size_t)3) + 4;
	l.ldh = (((size_t)H + 3) & ~(size_t)3) + 4;
	l.ld2 = ((O + 3) & ~(size_t)3) + 4;
	l.chunks = ((size_t)n + BSR_CONTEXT_CHUNK - 1) / BSR_CONTEXT_CHUNK;
	l.tot = H * D + H + (int)O * H + (int)O;
	l.off_hid = (size_t)n * l.ldx;
	l.off_dp1 = l.off_hid + (size_t)n * l.ldh;
	l.off_dp2 = l.off_dp1 + (size_t)n * l.ldh;
	l.off_partials = l.off_dp2 + (size_t)n * l.ld2;
	l.floats = l.off_partials + l.chunks * (size_t)l.tot + 64;
	return l;
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
				Hs[(j0 + jj) * CTX_P + t.lane] = heads_relu(acc[jj]);
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

__device__ __forceinline__ float step_size(float q, float adj) { return q * (1.0f + heads_tanh(adj)); }

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
			dst[idx] = qq + heads_tanh(x - qq) * q;
		}
	}
}

struct ContextUpstreams {
	const float *g_context, *g_q;
	const float* g_out[3];
	const float* noise[3];
};

__global__ void __launch_bounds__(CTX_MAX_THREADS) k_context_bwd_rows(ContextArgs a, ContextUpstreams u, float* __restrict__ d_enc,
                                                                      ContextRowScratch rs)
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
				const float tn = heads_tanh(adj[c]);
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

struct ContextSumArgs {
	int n, D, H, O, tot;
	const float *x, *hid, *dp1, *dp2;
	size_t ldx, ldh, ld2;
	float* partials;
};

// Element order of a partial (and of k_context_wsum): W1 [H, D], b1 [H], W2 [O, H], b2 [O].  A thread owns a 4 x 4 block
// of one weight matrix (and, in the first column of blocks, four bias elements).
__global__ void __launch_bounds__(CTX_SUM_BLOCK) k_context_wgrad(ContextSumArgs s)
{
	const int D = s.D, H = s.H, O = s.O;
	int u = blockIdx.y * CTX_SUM_BLOCK + threadIdx.x;
	const int KB1 = (D + 3) >> 2, JB1 = (H + 3) >> 2, KB2 = (H + 3) >> 2, JB2 = (O + 3) >> 2;
	const float *A, *B;
	size_t lda, ldb;
	int jv, kv, out, outld, bout, kb;
	if (u < JB1 * KB1) {
		const int jb = u / KB1;
		kb = u - jb * KB1;
		A = s.dp1 + 4 * jb; lda = s.ldh;
		B = s.x + 4 * kb; ldb = s.ldx;
		jv = H - 4 * jb; kv = D - 4 * kb;
		out = 4 * jb * D + 4 * kb; outld = D;
		bout = H * D + 4 * jb;
	} else {
		u -= JB1 * KB1;
		if (u >= JB2 * KB2) return;
		const int jb = u / KB2;
		kb = u - jb * KB2;
		A = s.dp2 + 4 * jb; lda = s.ld2;
		B = s.hid + 4 * kb; ldb = s.ldh;
		jv = O - 4 * jb; kv = H - 4 * kb;
		out = H * D + H + 4 * jb * H + 4 * kb; outld = H;
		bout = H * D + H + O * H + 4 * jb;
	}
	const size_t r0 = (size_t)blockIdx.x * BSR_CONTEXT_CHUNK;
	const size_t r1 = r0 + BSR_CONTEXT_CHUNK < (size_t)s.n ? r0 + BSR_CONTEXT_CHUNK : (size_t)s.n;
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

__global__ void __launch_bounds__(CTX_SUM_BLOCK) k_context_wsum(const float* __restrict__ partials, size_t chunks, int tot, int D,
                                                                int H, int O, bsr_context_weight_grads dw)
{
	int t = blockIdx.x * CTX_SUM_BLOCK + threadIdx.x;
	if (t >= tot) return;
	double sum = (double)partials[t];
	for (size_t c = 1; c < chunks; c++) sum = sum + (double)partials[c * (size_t)tot + t];
	float* p;
	if (t < H * D) p = dw.w1;
	else if ((t -= H * D) < H) p = dw.b1;
	else if ((t -= H) < O * H) p = dw.w2;
	else {
		t -= O * H;
		p = dw.b2;
	}
	if (p) p[t] = (float)sum;
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

// A workgroup's LDS is dynamic: refuse what the device cannot give one workgroup, and ask for more than the default
// 64 KiB once per kernel and DEVICE (not per call).  Two host threads that meet here both ask, which is harmless: the
// state is atomic and both store the same answer.
#define CTX_MAX_DEVICES 64
template <typename Kern>
static int context_lds(const char* who, Kern kern, size_t bytes)
{
	static std::atomic<int> device_lds[CTX_MAX_DEVICES];   // 0 not asked yet, else the device's LDS bytes per workgroup
	static std::atomic<int> state[CTX_MAX_DEVICES];        // (one array per kernel type) 0 not asked yet, 1 granted, -1 refused
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0) return fail("%s: no current device", who);
	const bool tracked = dev < CTX_MAX_DEVICES;
	int have = tracked ? device_lds[dev].load(std::memory_order_relaxed) : 0;
	if (have == 0) {
		if (hipDeviceGetAttribute(&have, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || have <= 0)
			return fail("%s: cannot read the device's LDS size", who);
		if (tracked) device_lds[dev].store(have, std::memory_order_relaxed);
	}
	if (bytes > (size_t)have)
		return fail("%s: a workgroup needs %zu bytes of LDS, the device gives one %d", who, bytes, have);
	if (bytes <= 64 * 1024) return 0;
	int st = tracked ? state[dev].load(std::memory_order_relaxed) : 0;
	if (st == 0) {
		st = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, have) == hipSuccess ? 1 : -1;
		if (tracked) state[dev].store(st, std::memory_order_relaxed);
	}
	if (st < 0) return fail("%s: cannot reserve %zu bytes of LDS", who, bytes);
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
	if (context_lds(who, k_context_fwd, lds)) return 1;
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
	if (context_lds(who, k_context_quantise, lds)) return 1;
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
	bsr_context_weight_grads grads = {};
	if (dw) grads = *dw;
	const bool sums = grads.w1 || grads.b1 || grads.w2 || grads.b2;
	if (((uintptr_t)grads.w1 | (uintptr_t)grads.b1 | (uintptr_t)grads.w2 | (uintptr_t)grads.b2) & 3)
		return fail("%s: weight gradients must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const size_t O = (size_t)a.O;
	if (n == 0) {
		float* p[4] = {grads.w1, grads.b1, grads.w2, grads.b2};
		const size_t count[4] = {(size_t)H * D, (size_t)H, O * H, O};
		for (int i = 0; i < 4; i++)
			if (p[i] && hipMemsetAsync(p[i], 0, count[i] * sizeof(float), st) != hipSuccess) return fail("%s: memset failed", who);
		return 0;
	}
	if (sums && !scratch) return fail("%s: the weight gradients need the scratch", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	const ContextLayout l = context_layout(n, D, H, F, K);
	ContextRowScratch rs = {};
	float* base = (float*)scratch;
	if (sums) {
		rs.x = base; rs.hid = base + l.off_hid; rs.dp1 = base + l.off_dp1; rs.dp2 = base + l.off_dp2;
		rs.ldx = l.ldx; rs.ldh = l.ldh; rs.ld2 = l.ld2;
	}
	const size_t lds = ((size_t)D + H + O) * CTX_P * sizeof(float);
	if (context_lds(who, k_context_bwd_rows, lds)) return 1;
	hipLaunchKernelGGL(k_context_bwd_rows, dim3(context_blocks(n)), dim3(CTX_T * CTX_BWD_WAVES), lds, st, a, u, d_enc, rs);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	if (!sums) return 0;
	ContextSumArgs s;
	s.n = n; s.D = D; s.H = H; s.O = a.O; s.tot = l.tot;
	s.x = rs.x; s.hid = rs.hid; s.dp1 = rs.dp1; s.dp2 = rs.dp2;
	s.ldx = l.ldx; s.ldh = l.ldh; s.ld2 = l.ld2;
	s.partials = base + l.off_partials;
	const int units = ((H + 3) / 4) * ((D + 3) / 4) + ((a.O + 3) / 4) * ((H + 3) / 4);
	hipLaunchKernelGGL(k_context_wgrad, dim3((unsigned)l.chunks, (unsigned)((units + CTX_SUM_BLOCK - 1) / CTX_SUM_BLOCK)),
	                   dim3(CTX_SUM_BLOCK), 0, st, s);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	hipLaunchKernelGGL(k_context_wsum, dim3((unsigned)((l.tot + CTX_SUM_BLOCK - 1) / CTX_SUM_BLOCK)), dim3(CTX_SUM_BLOCK), 0, st,
	                   s.partials, l.chunks, l.tot, D, H, a.O, grads);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
