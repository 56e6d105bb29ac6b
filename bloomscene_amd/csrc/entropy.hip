// The rate term of BloomScene's loss for gfx950 (include/bloomscene_entropy.h): Entropy_gaussian.forward and Low_bound
// (utils/entropy_models.py:10-50, "EM"), with the row selection, the mask and the sums of
// gaussian_renderer/__init__.py:100-127 ("GR") folded in.
//
//   k_entropy_fwd   bits (times the weight) of every element of every chosen row; optionally their sum and the count
//   k_entropy_bwd   the gradient to x, mean, scale, q and the weight, recomputed from the operands
//
// LANE MAPPING.  A row belongs to a group of G = 2^lg lanes, G the power of two >= C / r (at most 64, so a group never
// leaves its wave); a workgroup of 256 threads holds 256 / G rows.  Lane t of the group walks the weight entries
// t, t + G, ... and the r columns of each entry in order, so the sum over the columns of one weight entry stays inside one
// lane; the sum over a row (the gradient of a per-row q) is per lane in column order, then a butterfly over the
// group.  A row that is not chosen is left (or zero-filled) before any operand is loaded.
// SUMS.  total, count and the gradient of a single q: per thread in fp64 in index order, then grid_sum.h (which states
// the order), rounded once at the end.  The grid depends on (n, C, r) alone: bit-identical from run to run.
// No float atomics; the only atomic is the integer ticket.
// ARITHMETIC.  Per element two erf / erfc (one exp and a polynomial for a narrow bin), one log2 (forward), two exp, one
// expm1 and one division by l (backward), all from the device library: at BloomScene's shape (100 k rows, 5 % chosen, 86 columns over the three calls) that is
// 4.3e5 elements a step, and the kernels are bound by the rows they skip or zero-fill, not by these.
#include "common.h"
#include "grid_sum.h"
#include "../../include/bloomscene_entropy.h"

namespace bsr {

#define BSR_ENTROPY_BLOCK 256
#define BSR_ENTROPY_MAX_BLOCKS 4096   // more row tiles than this: grid-stride
#define BSR_ENTROPY_HEAD 256          // bytes of the scratch before the partials (the ticket)

struct EntropyOperands {
	int n, C, r, Cw, lg;       // Cw = C / r weight entries a row; 2^lg lanes a row
	long long tiles;           // row tiles of 256 >> lg rows
	const float *x, *mean, *scale, *q, *x_mean;
	long long xs, ms, ss;
	int q_mode;
	const unsigned char* rows;
	const float* w;
};

// scratch: [0, 4) the ticket; from BSR_ENTROPY_HEAD two fp64 per workgroup (the sum, then the chosen rows -- a count
// carried in fp64 is exact: it and every partial sum of it are integers below 2^31)
struct EntropyScratch {
	unsigned* ticket;
	double* psum;
};

static unsigned entropy_lg(int Cw)
{
	unsigned lg = 0;
	while (lg < 6 && (1 << lg) < Cw) lg++;
	return lg;
}
static long long entropy_tiles(int n, unsigned lg)
{
	const long long R = BSR_ENTROPY_BLOCK >> lg;
	return ((long long)n + R - 1) / R;
}
static unsigned entropy_blocks(long long tiles)
{
	return (unsigned)(tiles < 1 ? 1 : (tiles < BSR_ENTROPY_MAX_BLOCKS ? tiles : BSR_ENTROPY_MAX_BLOCKS));
}
static EntropyScratch entropy_scratch(void* scratch)
{
	EntropyScratch s;
	s.ticket = (unsigned*)scratch;
	s.psum = (double*)((char*)scratch + BSR_ENTROPY_HEAD);
	return s;
}

// everything about one element both kernels need
struct EntropyElement {
	float tu, tl, s, c, qv;   // the two arguments of Phi, the floored scale, xc - mean
	float D;                  // upper - lower, signed
	bool in_bounds, scale_ok;
};

// Phi(tu) - Phi(tl) with m = (tu + tl) / 2 and d = (tu - tl) / 2 given (c / s and q / 2s: no difference taken).
// A narrow bin, |d| <= 1/4: the integral of phi over [m - d, m + d] expanded at m,
//   2 d phi(m) sum_k d^2k He_2k(m) / (2k + 1)!,  k = 0 .. 4
// -- any difference of two cdf values there cancels to d times their size, and the gradient of q is ~ 1 / q, largest exactly
// there.  The first term left out is d^10 He_10(m) / 11!: below 3e-7 of the sum for |m| <= 6 (and at |m| = 6 the
// likelihood of such a bin is under the floor).  Wider bins: from the side where neither term is near 1.
// For |m| >= 16 the narrow bin is a zero with the sign of d: expf(-u / 2) is exactly 0 from u = 208 on, so every
// non-zero result is untouched, while he6 and he8 overflow from |m| ~ 6.6e4 on and 0 * inf would be a NaN (an infinite
// m included; d = 0 gives 0 for every m).
// A NaN argument fails the first two tests and ends up in the series or in an erf: NaN.
__device__ __forceinline__ float cdf_difference(float tu, float tl, float m, float d)
{
	if (fabsf(d) <= 0.25f) {
		const float u = m * m, d2 = d * d;
		if (u >= 256.0f) return d * 0.0f;
		const float he2 = u - 1.0f;
		const float he4 = (u - 6.0f) * u + 3.0f;
		const float he6 = ((u - 15.0f) * u + 45.0f) * u - 15.0f;
		const float he8 = (((u - 28.0f) * u + 210.0f) * u - 420.0f) * u + 105.0f;
		const float sum = 1.0f + d2 * (he2 * (1.0f / 6.0f) + d2 * (he4 * (1.0f / 120.0f) +
		                  d2 * (he6 * (1.0f / 5040.0f) + d2 * (he8 * (1.0f / 362880.0f)))));
		return (2.0f * d) * (expf(-0.5f * u) * 0.39894228040143267794f) * sum;
	}
	const float k = 0.70710678118654752440f;
	const bool up = tu >= tl;
	const float a = (up ? tl : tu) * k, b = (up ? tu : tl) * k;   // a <= b
	float r;
	if (a >= 0.0f) r = 0.5f * (erfcf(a) - erfcf(b));
	else if (b <= 0.0f) r = 0.5f * (erfcf(-b) - erfcf(-a));
	else r = 0.5f * (erff(b) - erff(a));
	return up ? r : -r;
}

__device__ __forceinline__ EntropyElement entropy_element(float xv, float mv, float sv, float qv, float xm)
{
	EntropyElement e;
	const float span = 15000.0f * qv;
	const float lo = xm - span, hi = xm + span;
	float xc = xv < lo ? lo : xv;
	xc = xc > hi ? hi : xc;
	e.in_bounds = xv >= lo && xv <= hi;
	e.scale_ok = sv >= 1e-9f;
	e.s = sv < 1e-9f ? 1e-9f : sv;
	e.c = xc - mv;
	e.qv = qv;
	const float h = 0.5f * qv;
	e.tu = (e.c + h) / e.s;
	e.tl = (e.c - h) / e.s;
	e.D = cdf_difference(e.tu, e.tl, e.c / e.s, h / e.s);
	return e;
}

__device__ __forceinline__ float entropy_bits(float l) { return -log2f(l < 1e-6f ? 1e-6f : l); }

__device__ __forceinline__ double group_sum(double v, int G)   // over the G lanes of a row group: every lane gets it
{
	for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

__global__ void __launch_bounds__(BSR_ENTROPY_BLOCK) k_entropy_fwd(EntropyOperands a, float* __restrict__ bits,
                                                                   float* __restrict__ likelihood,
                                                                   float* __restrict__ total, long long* __restrict__ count,
                                                                   EntropyScratch sc)
{
	const int G = 1 << a.lg, lane = threadIdx.x & (G - 1), rib = threadIdx.x >> a.lg, R = BSR_ENTROPY_BLOCK >> a.lg;
	const float xm = a.x_mean[0];
	double sums[2] = {0.0, 0.0};   // the bits, the chosen rows
	for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
		const long long i = tile * R + rib;
		if (i >= (long long)a.n) continue;
		if (a.rows && !a.rows[i]) {
			for (int j = lane; j < a.C; j += G) {
				if (bits) bits[i * a.C + j] = 0.0f;
				if (likelihood) likelihood[i * a.C + j] = 0.0f;
			}
			continue;
		}
		if (lane == 0) sums[1] += 1.0;
		const float qrow = a.q_mode == BSR_ENTROPY_Q_SINGLE ? a.q[0] : (a.q_mode == BSR_ENTROPY_Q_ROW ? a.q[i] : 0.0f);
		for (int jw = lane; jw < a.Cw; jw += G) {
			const float wv = a.w ? a.w[i * a.Cw + jw] : 1.0f;
			for (int k = 0; k < a.r; k++) {
				const int j = jw * a.r + k;
				const float qv = a.q_mode == BSR_ENTROPY_Q_ELEMENT ? a.q[i * a.C + j] : qrow;
				const EntropyElement e = entropy_element(a.x[i * a.xs + j], a.mean[i * a.ms + j], a.scale[i * a.ss + j], qv, xm);
				const float l = fabsf(e.D);
				const float b = entropy_bits(l);
				const float term = a.w ? b * wv : b;
				if (bits) bits[i * a.C + j] = term;
				if (likelihood) likelihood[i * a.C + j] = l;
				sums[0] += (double)term;
			}
		}
	}
	if (!total && !count) return;   // (uniform: no sums asked for)
	if (grid_sum<2, BSR_ENTROPY_BLOCK>(sums, sc.ticket, sc.psum)) {
		if (total) total[0] = (float)sums[0];
		if (count) count[0] = (long long)sums[1] * (long long)a.C;
	}
}

__global__ void __launch_bounds__(BSR_ENTROPY_BLOCK) k_entropy_bwd(EntropyOperands a, const float* __restrict__ g, int g_mode,
                                                                   float* __restrict__ dx, float* __restrict__ dmean,
                                                                   float* __restrict__ dscale, float* __restrict__ dq,
                                                                   float* __restrict__ dw, EntropyScratch sc)
{
	const int G = 1 << a.lg, lane = threadIdx.x & (G - 1), rib = threadIdx.x >> a.lg, R = BSR_ENTROPY_BLOCK >> a.lg;
	const float xm = a.x_mean[0];
	const float g_single = g_mode == BSR_ENTROPY_G_SINGLE ? g[0] : 0.0f;
	const bool dq_row = dq && a.q_mode != BSR_ENTROPY_Q_ELEMENT;
	double acc[1] = {0.0};   // the gradient of a single q
	for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
		const long long i = tile * R + rib;
		if (i >= (long long)a.n) continue;
		if (a.rows && !a.rows[i]) {
			for (int j = lane; j < a.C; j += G) {
				if (dx) dx[i * a.C + j] = 0.0f;
				if (dmean) dmean[i * a.C + j] = 0.0f;
				if (dscale) dscale[i * a.C + j] = 0.0f;
				if (dq && a.q_mode == BSR_ENTROPY_Q_ELEMENT) dq[i * a.C + j] = 0.0f;
			}
			if (dw) for (int jw = lane; jw < a.Cw; jw += G) dw[i * a.Cw + jw] = 0.0f;
			if (dq && a.q_mode == BSR_ENTROPY_Q_ROW && lane == 0) dq[i] = 0.0f;
			continue;
		}
		const float qrow = a.q_mode == BSR_ENTROPY_Q_SINGLE ? a.q[0] : (a.q_mode == BSR_ENTROPY_Q_ROW ? a.q[i] : 0.0f);
		double dq_lane = 0.0;
		for (int jw = lane; jw < a.Cw; jw += G) {
			const float wv = a.w ? a.w[i * a.Cw + jw] : 1.0f;
			float dw_entry = 0.0f;
			for (int k = 0; k < a.r; k++) {
				const int j = jw * a.r + k;
				const float qv = a.q_mode == BSR_ENTROPY_Q_ELEMENT ? a.q[i * a.C + j] : qrow;
				const EntropyElement e = entropy_element(a.x[i * a.xs + j], a.mean[i * a.ms + j], a.scale[i * a.ss + j], qv, xm);
				const float l = fabsf(e.D);
				const float g_out = g_mode == BSR_ENTROPY_G_SINGLE ? g_single : g[i * a.C + j];
				dw_entry += g_out * entropy_bits(l);
				const float g_bits = a.w ? g_out * wv : g_out;
				const float gl = l >= 1e-6f ? -g_bits / (l * 0.69314718055994530942f) : 0.0f;
				const float sg = e.D > 0.0f ? 1.0f : (e.D < 0.0f ? -1.0f : 0.0f);
				const float ga = gl * sg;
				const float inv = 0.39894228040143267794f / e.s;
				const float du = expf(-0.5f * e.tu * e.tu) * inv, dl = expf(-0.5f * e.tl * e.tl) * inv;
				const float qs = e.qv / e.s;
				const float ex = (e.c / e.s) * qs;   // (tu^2 - tl^2) / 2: phi(tu) = phi(tl) exp(-ex)
				float diff, tdiff;                   // du - dl, tu du - tl dl
				if (ex <= 0.0f) {
					diff = -(du * expm1f(ex));
					tdiff = e.tl * diff + qs * du;
				} else {
					diff = dl * expm1f(-ex);
					tdiff = e.tu * diff + qs * dl;
				}
				// below the floor nothing flows, whatever tu and tl are (an overflowed tu makes tdiff inf * 0)
				const bool open = l >= 1e-6f;
				const float gd = open ? ga * diff : 0.0f;
				if (dx) dx[i * a.C + j] = e.in_bounds ? gd : 0.0f;
				if (dmean) dmean[i * a.C + j] = -gd;
				if (dscale) dscale[i * a.C + j] = e.scale_ok && open ? -(ga * tdiff) : 0.0f;
				const float dqv = open ? ga * ((du + dl) * 0.5f) : 0.0f;
				if (dq && a.q_mode == BSR_ENTROPY_Q_ELEMENT) dq[i * a.C + j] = dqv;
				dq_lane += (double)dqv;
			}
			if (dw) dw[i * a.Cw + jw] = dw_entry;
		}
		if (dq_row) {
			const double row = group_sum(dq_lane, G);
			if (lane == 0) {
				if (a.q_mode == BSR_ENTROPY_Q_ROW) dq[i] = (float)row;
				else acc[0] += row;
			}
		}
	}
	if (!(dq && a.q_mode == BSR_ENTROPY_Q_SINGLE)) return;   // (uniform)
	if (grid_sum<1, BSR_ENTROPY_BLOCK>(acc, sc.ticket, sc.psum)) dq[0] = (float)acc[0];
}

// the checks both entry points share; fills the operands
static int entropy_operands(const char* who, int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                            const float* scale, long long ss, const float* q, int q_mode, const float* x_mean,
                            const unsigned char* rows, const float* w, EntropyOperands& a)
{
	if (n < 0 || C < 1 || r < 1 || C % r != 0) return fail("%s: need n >= 0, C >= 1, r >= 1 and C %% r == 0 (got %d, %d, %d)", who, n, C, r);
	if ((long long)n * C >= (1LL << 40)) return fail("%s: n * C must be below 2^40 (got %d * %d)", who, n, C);
	if (q_mode < BSR_ENTROPY_Q_SINGLE || q_mode > BSR_ENTROPY_Q_ELEMENT) return fail("%s: unknown q_mode %d", who, q_mode);
	if (!w && r != 1) return fail("%s: r must be 1 without a weight (got %d)", who, r);
	if (xs < C || ms < C || ss < C) return fail("%s: row strides must be >= C = %d (got %lld, %lld, %lld)", who, C, xs, ms, ss);
	if (n > 0 && (!x || !mean || !scale || !q || !x_mean)) return fail("%s: NULL operand", who);
	if (((uintptr_t)x | (uintptr_t)mean | (uintptr_t)scale | (uintptr_t)q | (uintptr_t)x_mean | (uintptr_t)w) & 3)
		return fail("%s: operands must be 4-byte aligned", who);
	a.n = n; a.C = C; a.r = r; a.Cw = C / r;
	a.lg = (int)entropy_lg(a.Cw);
	a.tiles = entropy_tiles(n, (unsigned)a.lg);
	a.x = x; a.mean = mean; a.scale = scale; a.q = q; a.x_mean = x_mean;
	a.xs = xs; a.ms = ms; a.ss = ss;
	a.q_mode = q_mode;
	a.rows = rows;
	a.w = w;
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_entropy_scratch_bytes(int n, int C, int r)
{
	if (n < 0 || C < 1 || r < 1 || C % r != 0) return 0;
	const unsigned blocks = entropy_blocks(entropy_tiles(n, entropy_lg(C / r)));
	return align_up(BSR_ENTROPY_HEAD + (size_t)blocks * 2 * sizeof(double), 256);
}

int bsr_entropy_forward(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                        const float* scale, long long ss, const float* q, int q_mode, const float* x_mean,
                        const unsigned char* rows, const float* w, float* bits, float* likelihood, float* total,
                        long long* count, void* scratch, void* stream)
{
	const char* who = "bsr_entropy_forward";
	EntropyOperands a;
	if (entropy_operands(who, n, C, r, x, xs, mean, ms, scale, ss, q, q_mode, x_mean, rows, w, a)) return 1;
	if (((uintptr_t)bits | (uintptr_t)likelihood | (uintptr_t)total) & 3) return fail("%s: outputs must be 4-byte aligned", who);
	const bool sums = total || count;
	if (sums && !scratch) return fail("%s: total and count need the scratch", who);
	if (((uintptr_t)scratch | (uintptr_t)count) & 7) return fail("%s: scratch and count must be 8-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) {
		if (total && hipMemsetAsync(total, 0, sizeof(float), st) != hipSuccess) return fail("%s: memset failed", who);
		if (count && hipMemsetAsync(count, 0, sizeof(long long), st) != hipSuccess) return fail("%s: memset failed", who);
		return 0;
	}
	const unsigned blocks = entropy_blocks(a.tiles);
	EntropyScratch sc = {};
	if (sums) {
		sc = entropy_scratch(scratch);
		if (hipMemsetAsync(sc.ticket, 0, sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	}
	hipLaunchKernelGGL(k_entropy_fwd, dim3(blocks), dim3(BSR_ENTROPY_BLOCK), 0, st, a, bits, likelihood, total, count, sc);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_entropy_backward(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                         const float* scale, long long ss, const float* q, int q_mode, const float* x_mean,
                         const unsigned char* rows, const float* w, const float* g, int g_mode, float* dx, float* dmean,
                         float* dscale, float* dq, float* dw, void* scratch, void* stream)
{
	const char* who = "bsr_entropy_backward";
	EntropyOperands a;
	if (entropy_operands(who, n, C, r, x, xs, mean, ms, scale, ss, q, q_mode, x_mean, rows, w, a)) return 1;
	if (g_mode != BSR_ENTROPY_G_DENSE && g_mode != BSR_ENTROPY_G_SINGLE) return fail("%s: unknown g_mode %d", who, g_mode);
	if (dw && !w) return fail("%s: dw without a weight", who);
	if (((uintptr_t)g | (uintptr_t)dx | (uintptr_t)dmean | (uintptr_t)dscale | (uintptr_t)dq | (uintptr_t)dw) & 3)
		return fail("%s: g and the gradients must be 4-byte aligned", who);
	const bool sums = dq && q_mode == BSR_ENTROPY_Q_SINGLE;
	if (sums && !scratch) return fail("%s: the gradient of a single q needs the scratch", who);
	if ((uintptr_t)scratch & 7) return fail("%s: scratch must be 8-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	if (n == 0) {
		if (sums && hipMemsetAsync(dq, 0, sizeof(float), st) != hipSuccess) return fail("%s: memset failed", who);
		return 0;
	}
	if (!g) return fail("%s: NULL g", who);
	const unsigned blocks = entropy_blocks(a.tiles);
	EntropyScratch sc = {};
	if (sums) {
		sc = entropy_scratch(scratch);
		if (hipMemsetAsync(sc.ticket, 0, sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	}
	hipLaunchKernelGGL(k_entropy_bwd, dim3(blocks), dim3(BSR_ENTROPY_BLOCK), 0, st, a, g, g_mode, dx, dmean, dscale, dq, dw, sc);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
