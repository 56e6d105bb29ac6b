// The weight-gradient sums of the row-per-lane MLP units (mlp_wgrad.h): the two kernels and the host side of a backward
// entry point around them.  The grid is a function of the shape alone.
#include "mlp_wgrad.h"
#include "../../include/bloomscene_heads.h"
#include "../../include/bloomscene_context.h"

namespace bsr {

static_assert(BSR_HEADS_CHUNK == MLP_WGRAD_CHUNK && BSR_CONTEXT_CHUNK == MLP_WGRAD_CHUNK, "the public headers promise this range length");

__global__ void __launch_bounds__(MLP_WGRAD_BLOCK) k_mlp_wgrad(MlpProducts t, int n, int tot, float* __restrict__ partials)
{
	int u = blockIdx.y * MLP_WGRAD_BLOCK + threadIdx.x;
	// the unit's product: the last one whose first unit is <= u (the unit counts are uniform: scalar loads, no branch)
	int i = 0, first = 0, end = 0;
#pragma unroll
	for (int k = 0; k < MLP_WGRAD_MAX_PRODUCTS; k++) {
		end += ((t.p[k].J + 3) >> 2) * ((t.p[k].Kd + 3) >> 2);
		if (u >= end) {
			i = k + 1;
			first = end;
		}
	}
	if (i == MLP_WGRAD_MAX_PRODUCTS) return;
	u -= first;
	const MlpProduct q = t.p[i];
	const int Kd = q.Kd, KB = (Kd + 3) >> 2;
	const int jb = u / KB, kb = u - jb * KB;
	const float *A = q.A + 4 * jb, *B = q.B + 4 * kb;
	const size_t lda = q.lda, ldb = q.ldb;
	const int jv = q.J - 4 * jb, kv = Kd - 4 * kb;
	const int out = q.out + 4 * jb * Kd + 4 * kb, bout = q.bout + 4 * jb;
	const size_t r0 = (size_t)blockIdx.x * MLP_WGRAD_CHUNK;
	const size_t r1 = r0 + MLP_WGRAD_CHUNK < (size_t)n ? r0 + MLP_WGRAD_CHUNK : (size_t)n;
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
	float* P = partials + (size_t)blockIdx.x * tot;
#pragma unroll
	for (int jj = 0; jj < 4; jj++) {
		if (jj >= jv) continue;
#pragma unroll
		for (int kk = 0; kk < 4; kk++)
			if (kk < kv) P[out + jj * Kd + kk] = (float)acc[jj][kk];
		if (kb == 0) P[bout + jj] = (float)ab[jj];
	}
}

__global__ void __launch_bounds__(MLP_WGRAD_BLOCK) k_mlp_wsum(const float* __restrict__ partials, size_t chunks, MlpSegments d)
{
	const int t = blockIdx.x * MLP_WGRAD_BLOCK + threadIdx.x;
	if (t >= d.tot) return;
	double sum = (double)partials[t];
	for (size_t c = 1; c < chunks; c++) sum = sum + (double)partials[c * (size_t)d.tot + t];
	int i = 0;
	while (t >= d.s[i].first + d.s[i].count) i++;   // (the segments cover [0, tot))
	if (d.s[i].dst) d.s[i].dst[t - d.s[i].first] = (float)sum;
}

bool mlp_wgrad_asked(const MlpSegments& d)
{
	for (int i = 0; i < d.count; i++)
		if (d.s[i].dst) return true;
	return false;
}

int mlp_wgrad_check(const char* who, const MlpSegments& d)
{
	for (int i = 0; i < d.count; i++)
		if ((uintptr_t)d.s[i].dst & 3) return fail("%s: weight gradients must be 4-byte aligned", who);
	return 0;
}

int mlp_wgrad_zero(const char* who, const MlpSegments& d, hipStream_t st)
{
	for (int i = 0; i < d.count; i++)
		if (d.s[i].dst && hipMemsetAsync(d.s[i].dst, 0, (size_t)d.s[i].count * sizeof(float), st) != hipSuccess)
			return fail("%s: memset failed", who);
	return 0;
}

int mlp_wgrad_carve(const char* who, const MlpWgradLayout& l, bool sums, void* scratch, MlpRowScratch& rs)
{
	if (sums && !scratch) return fail("%s: the weight gradients need the scratch", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	float* base = (float*)scratch;
	rs = {};
	if (sums) rs = {base, base + l.off_hid, base + l.off_dp1, base + l.off_dp2, l.ldx, l.ldh, l.ld2};
	return 0;
}

int mlp_wgrad_sums(const char* who, const MlpProducts& pr, const MlpSegments& d, int n, const MlpWgradLayout& l, void* scratch,
                   hipStream_t st)
{
	float* partials = (float*)scratch + l.off_partials;
	int units = 0;
	for (int i = 0; i < pr.count; i++) units += ((pr.p[i].J + 3) / 4) * ((pr.p[i].Kd + 3) / 4);
	hipLaunchKernelGGL(k_mlp_wgrad, dim3((unsigned)l.chunks, (unsigned)((units + MLP_WGRAD_BLOCK - 1) / MLP_WGRAD_BLOCK)),
	                   dim3(MLP_WGRAD_BLOCK), 0, st, pr, n, d.tot, partials);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	hipLaunchKernelGGL(k_mlp_wsum, dim3((unsigned)((d.tot + MLP_WGRAD_BLOCK - 1) / MLP_WGRAD_BLOCK)), dim3(MLP_WGRAD_BLOCK), 0, st,
	                   partials, l.chunks, d);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // namespace bsr
