// The fused Adam step for gfx950 (include/bloomscene_adam.h): every tensor of the optimizer in ONE launch, the
// multi-tensor-apply shape.  The descriptors -- four pointers, the element count and the per-tensor scalars of up to
// BSR_ADAM_MAX_TENSORS tensors -- and a prefix array of chunk counts travel in the kernel-argument block (under HIP's 4 KB),
// so nothing is copied to the device and nothing is allocated.
//
// k_adam<CAP>     a 256-thread workgroup owns one chunk of BSR_ADAM_CHUNK elements of one tensor.  It finds (tensor, chunk)
//                 by a binary search of blockIdx.x in the prefix array: wave-uniform, so the lookup, the pointers and the
//                 per-tensor scalars stay in scalar registers.  A tensor whose four pointers are all 16-byte aligned moves
//                 through 16-byte loads of p, g, m, v -- all 16 of a thread issued before the first use -- and 16-byte
//                 stores of p, m, v; a full chunk takes them unpredicated.  Any other tensor, and the last numel % 4
//                 elements of an aligned one, go element by element.  No LDS, no atomics, no scratch.
//                 CAP: lr and t - 1 are read from the device and ss, bc2s formed here, per workgroup, by the host's own code.
// k_adam_advance  the capturable form's second launch: one thread per tensor adds 1 to its step.
//
// BSR_ADAM_NT_G (an A/B define, docs/EXPERIMENTS.md): the gradient, dead after the step, is loaded non-temporally.
#include "common.h"
#include "errors.h"
#include "adam_bpow.h"
#include "../../include/bloomscene_adam.h"

#include <cmath>

namespace bsr {

#define BSR_ADAM_BLOCK 256
#define BSR_ADAM_VECS (BSR_ADAM_CHUNK / 4 / BSR_ADAM_BLOCK)   // 16-byte vectors of one array a thread moves
static_assert(BSR_ADAM_CHUNK % 1024 == 0, "a chunk is whole 16-byte vectors for every thread, and keeps 16-byte alignment");

typedef float f4 __attribute__((ext_vector_type(4)));

struct AdamScalars {
	double beta1, beta2;   // CAP only: the bases of bpow
	float b2, w1, w2, eps;
};

template <bool CAP>
struct AdamPack;

template <>
struct AdamPack<false> {
	float* p[BSR_ADAM_MAX_TENSORS];
	const float* g[BSR_ADAM_MAX_TENSORS];
	float* m[BSR_ADAM_MAX_TENSORS];
	float* v[BSR_ADAM_MAX_TENSORS];
	float ss[BSR_ADAM_MAX_TENSORS];
	float bc2s[BSR_ADAM_MAX_TENSORS];
	int numel[BSR_ADAM_MAX_TENSORS];
	int start[BSR_ADAM_MAX_TENSORS + 1];   // first workgroup of each tensor; start[n] = the grid
};

template <>
struct AdamPack<true> {
	float* p[BSR_ADAM_MAX_TENSORS];
	const float* g[BSR_ADAM_MAX_TENSORS];
	float* m[BSR_ADAM_MAX_TENSORS];
	float* v[BSR_ADAM_MAX_TENSORS];
	const float* lr[BSR_ADAM_MAX_TENSORS];
	float* step[BSR_ADAM_MAX_TENSORS];
	int numel[BSR_ADAM_MAX_TENSORS];
	int start[BSR_ADAM_MAX_TENSORS + 1];
};

struct AdamSteps {
	float* step[BSR_ADAM_MAX_TENSORS];
};

static_assert(sizeof(AdamPack<true>) + sizeof(AdamScalars) + 16 <= 4096 && sizeof(AdamPack<false>) <= sizeof(AdamPack<true>),
              "the descriptors must fit the kernel-argument block");

// The function of the header, one element.  Built with -ffp-contract=off: every operation below is rounded once.
struct AdamCoef {
	float b2, w1, w2, eps, ss, bc2s;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamCoef& c)
{
	const float d = g - m;
	m = m + c.w1 * d;
	const float gg = g * g;
	v = c.b2 * v + c.w2 * gg;
	const float den = sqrtf(v) / c.bc2s + c.eps;
	p = p - c.ss * (m / den);
}

__device__ __forceinline__ f4 load_grad(const f4* g)
{
#ifdef BSR_ADAM_NT_G
	return __builtin_nontemporal_load(g);
#else
	return *g;
#endif
}

// n4 vectors of an aligned chunk; FULL: n4 == BSR_ADAM_VECS * BSR_ADAM_BLOCK, no predicate
template <bool FULL>
__device__ __forceinline__ void adam_vectors(f4* p, const f4* g, f4* m, f4* v, int n4, const AdamCoef& c)
{
	f4 P[BSR_ADAM_VECS], G[BSR_ADAM_VECS], M[BSR_ADAM_VECS], V[BSR_ADAM_VECS];
#pragma unroll
	for (int k = 0; k < BSR_ADAM_VECS; ++k) {
		const int i = threadIdx.x + k * BSR_ADAM_BLOCK;
		if (FULL || i < n4) {
			P[k] = p[i];
			G[k] = load_grad(g + i);
			M[k] = m[i];
			V[k] = v[i];
		}
	}
	// every load above is issued before the first use below: left to itself the scheduler sinks three quarters of them
	// behind the first vector's arithmetic
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int k = 0; k < BSR_ADAM_VECS; ++k) {
		const int i = threadIdx.x + k * BSR_ADAM_BLOCK;
		if (FULL || i < n4) {
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				float pj = P[k][j], mj = M[k][j], vj = V[k][j];
				adam_elem(pj, G[k][j], mj, vj, c);
				P[k][j] = pj;
				M[k][j] = mj;
				V[k][j] = vj;
			}
			p[i] = P[k];
			m[i] = M[k];
			v[i] = V[k];
		}
	}
}

template <bool CAP>
__global__ __launch_bounds__(BSR_ADAM_BLOCK) void k_adam(const AdamPack<CAP> a, const AdamScalars s, int n)
{
	const int b = blockIdx.x;
	// the last tensor t with start[t] <= b: a tensor without elements has start[t] == start[t + 1] and is never found
	int t = 0, hi = n;
	while (hi - t > 1) {
		const int mid = (t + hi) >> 1;
		if (a.start[mid] <= b) t = mid;
		else hi = mid;
	}
	AdamCoef c;
	c.b2 = s.b2;
	c.w1 = s.w1;
	c.w2 = s.w2;
	c.eps = s.eps;
	if constexpr (CAP) {
		const float lr = *a.lr[t];
		const long long step = (long long)*a.step[t] + 1;   // the device holds t - 1
		adam_step_scalars((double)lr, s.beta1, s.beta2, step, &c.ss, &c.bc2s);
	} else {
		c.ss = a.ss[t];
		c.bc2s = a.bc2s[t];
	}
	const int base = (b - a.start[t]) * BSR_ADAM_CHUNK;   // < numel < 2^31
	const int count = min(BSR_ADAM_CHUNK, a.numel[t] - base);
	float* p = a.p[t] + base;
	const float* g = a.g[t] + base;
	float* m = a.m[t] + base;
	float* v = a.v[t] + base;
	const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
	int done = 0;
	if (aligned) {
		if (count == BSR_ADAM_CHUNK) {
			adam_vectors<true>((f4*)p, (const f4*)g, (f4*)m, (f4*)v, BSR_ADAM_CHUNK / 4, c);
			return;
		}
		adam_vectors<false>((f4*)p, (const f4*)g, (f4*)m, (f4*)v, count >> 2, c);
		done = count & ~3;
	}
	for (int i = done + threadIdx.x; i < count; i += BSR_ADAM_BLOCK) {
		float pi = p[i], mi = m[i], vi = v[i];
		adam_elem(pi, g[i], mi, vi, c);
		p[i] = pi;
		m[i] = mi;
		v[i] = vi;
	}
}

__global__ void k_adam_advance(const AdamSteps a, int n)
{
	const int i = threadIdx.x;
	if (i < n) *a.step[i] = *a.step[i] + 1.0f;
}

template <bool CAP>
static int launch_batch(const char* who, const bsr_adam_tensor* const* batch, int n, const AdamScalars& s, hipStream_t st)
{
	AdamPack<CAP> a;
	AdamSteps steps;
	long long blocks = 0;
	for (int k = 0; k < BSR_ADAM_MAX_TENSORS; ++k) {
		const bsr_adam_tensor* t = batch[k < n ? k : n - 1];   // the unused slots repeat the last tensor: never read
		a.p[k] = t->p;
		a.g[k] = t->g;
		a.m[k] = t->m;
		a.v[k] = t->v;
		a.numel[k] = k < n ? (int)t->numel : 0;
		a.start[k] = (int)blocks;
		if (k < n) blocks += (t->numel + BSR_ADAM_CHUNK - 1) / BSR_ADAM_CHUNK;
		if constexpr (CAP) {
			a.lr[k] = t->lr_dev;
			a.step[k] = t->step_dev;
			steps.step[k] = t->step_dev;
		} else {
			adam_step_scalars(t->lr, s.beta1, s.beta2, t->step, &a.ss[k], &a.bc2s[k]);
		}
	}
	a.start[BSR_ADAM_MAX_TENSORS] = (int)blocks;   // (64 tensors below 2^31 elements: at most 2^25 workgroups)
	hipLaunchKernelGGL((k_adam<CAP>), dim3((unsigned)blocks), dim3(BSR_ADAM_BLOCK), 0, st, a, s, n);
	if constexpr (CAP) hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(BSR_ADAM_MAX_TENSORS), 0, st, steps, n);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

int bsr_adam_max_tensors(void)
{
	return BSR_ADAM_MAX_TENSORS;
}

int bsr_adam_step(int n_tensors, const bsr_adam_tensor* tensors, double beta1, double beta2, double eps, void* stream)
{
	const char* who = "bsr_adam_step";
	g_err[0] = 0;
	if (n_tensors < 0) return fail("%s: need n_tensors >= 0 (got %d)", who, n_tensors);
	if (n_tensors > 0 && !tensors) return fail("%s: NULL tensor array", who);
	if (!std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps)) return fail("%s: beta1, beta2 and eps must be finite", who);
	if (beta1 < 0.0 || beta1 >= 1.0) return fail("%s: beta1 must be in [0, 1) (got %g)", who, beta1);
	if (beta2 < 0.0 || beta2 >= 1.0) return fail("%s: beta2 must be in [0, 1) (got %g)", who, beta2);
	if (eps < 0.0) return fail("%s: need eps >= 0 (got %g)", who, eps);
	int form = -1;   // 0 default, 1 capturable: the first tensor with elements decides
	for (int k = 0; k < n_tensors; ++k) {
		const bsr_adam_tensor& t = tensors[k];
		if (t.numel < 0 || t.numel >= (1ll << 31)) return fail("%s: tensor %d: numel must be in [0, 2^31) (got %lld)", who, k, t.numel);
		if (t.numel == 0) continue;
		if (!t.p || !t.g || !t.m || !t.v) return fail("%s: tensor %d: NULL buffer", who, k);
		if ((t.lr_dev == nullptr) != (t.step_dev == nullptr)) return fail("%s: tensor %d: lr_dev and step_dev come together", who, k);
		const int f = t.lr_dev ? 1 : 0;
		if (form < 0) form = f;
		if (f != form) return fail("%s: tensor %d: the default and the capturable form cannot share a call", who, k);
		if (!f) {
			if (!std::isfinite(t.lr)) return fail("%s: tensor %d: lr must be finite", who, k);
			if (t.step < 1) return fail("%s: tensor %d: need step >= 1 (got %lld)", who, k, t.step);
		}
	}
	if (form < 0) return 0;   // nothing has elements: no launch
	AdamScalars s;
	s.beta1 = beta1;
	s.beta2 = beta2;
	s.b2 = (float)beta2;
	s.w1 = (float)(1.0 - beta1);
	s.w2 = (float)(1.0 - beta2);
	s.eps = (float)eps;
	hipStream_t st = (hipStream_t)stream;
	const bsr_adam_tensor* batch[BSR_ADAM_MAX_TENSORS];
	int n = 0;
	for (int k = 0; k <= n_tensors; ++k) {
		if (k < n_tensors && tensors[k].numel > 0) batch[n++] = &tensors[k];
		if (n == BSR_ADAM_MAX_TENSORS || (k == n_tensors && n > 0)) {
			const int rc = form ? launch_batch<true>(who, batch, n, s, st) : launch_batch<false>(who, batch, n, s, st);
			if (rc) return rc;
			n = 0;
		}
	}
	return 0;
}

}  // extern "C"
