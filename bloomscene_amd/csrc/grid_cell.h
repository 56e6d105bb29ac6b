// The device functions the hash-grid units share (grid.hip: one table per call, include/bloomscene_grid.h; mix_grid.hip:
// the fused mixed 3D/2D binary encoding, include/bloomscene_mix_grid.h): the row rule, a row of F floats, the cell of one
// (point, level) with its 2^D corners, and the scale exponent of the backward's fixed-point rule.  Written once, so that
// the two units cannot drift apart: the fused unit is bit-equal to the single-table one by construction.
// "GC" = the reference's submodules/gridencoder/src/gridencoder.cu.
#pragma once
#include "common.h"

namespace bsr {

#define BSR_GRID_BLOCK 256
#define BSR_GRID_MAX_LEVELS 64

// GC:44-57: coherent hash (primes of instant-ngp), uint32 wrap-around
__device__ __forceinline__ uint32_t grid_prime(int d) { return d == 0 ? 1u : (d == 1 ? 2654435761u : 805459861u); }

// GC:62-88 without the feature factor: the row (relative to the level's first row) of grid point p
template <int D>
__device__ __forceinline__ uint32_t grid_row(const uint32_t (&p)[D], uint32_t hs, uint32_t res)
{
	uint32_t stride = 1, index = 0;
#pragma unroll
	for (int d = 0; d < D; d++) {
		if (stride > hs) break;
		index += p[d] * stride;
		stride *= res;
	}
	if (stride > hs) {
		index = 0;
#pragma unroll
		for (int d = 0; d < D; d++) index ^= p[d] * grid_prime(d);
	}
	return index % hs;
}

template <int F> struct Feat { float v[F]; };

// One row of F floats: one 8- or 16-byte load per 8 / 16 bytes (embeddings aligned to min(16, 4F): checked on entry)
template <int F>
__device__ __forceinline__ Feat<F> load_feat(const float* p)
{
	Feat<F> r;
	if constexpr (F == 1) {
		r.v[0] = p[0];
	} else if constexpr (F == 2) {
		const bsr_f32x2 a = *reinterpret_cast<const bsr_f32x2*>(p);
		r.v[0] = a.x; r.v[1] = a.y;
	} else {
#pragma unroll
		for (int k = 0; k < F; k += 4) {
			const bsr_f32x4 a = *reinterpret_cast<const bsr_f32x4*>(p + k);
			r.v[k] = a.x; r.v[k + 1] = a.y; r.v[k + 2] = a.z; r.v[k + 3] = a.w;
		}
	}
	return r;
}

template <int F>
__device__ __forceinline__ void store_feat(float* p, const Feat<F>& r)
{
	if constexpr (F == 1) {
		p[0] = r.v[0];
	} else if constexpr (F == 2) {
		bsr_f32x2 a; a.x = r.v[0]; a.y = r.v[1];
		*reinterpret_cast<bsr_f32x2*>(p) = a;
	} else {
#pragma unroll
		for (int k = 0; k < F; k += 4) {
			bsr_f32x4 a; a.x = r.v[k]; a.y = r.v[k + 1]; a.z = r.v[k + 2]; a.w = r.v[k + 3];
			*reinterpret_cast<bsr_f32x4*>(p + k) = a;
		}
	}
}

// The cell of one (point, level) and its 2^D corners: weights, inclusion, rows; wn_re.  GC:166-335.
template <int D>
struct Cell {
	float pos[D];
	uint32_t pg[D];
	float w[1 << D];
	uint32_t row[1 << D];
	bool ok[1 << D];
	float wn_re;
};

template <int D>
__device__ __forceinline__ void make_cell(const float (&x)[D], uint32_t hs, uint32_t res, long long rows_left, Cell<D>& c)
{
	const float scale = (float)(res - 2u);
#pragma unroll
	for (int d = 0; d < D; d++) {
		const float p = x[d] * scale + 0.5f;   // GC:183 (the double 0.5 gives the fp32 sum: p + 0.5 is exact in double)
		c.pg[d] = (uint32_t)floorf(p);
		c.pos[d] = p - (float)c.pg[d];
	}
	float wn = 0.0f;
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		float w = 1.0f;
		uint32_t p[D];
		bool ok = true;
#pragma unroll
		for (int d = 0; d < D; d++) {
			if (((k >> d) & 1) == 0) {
				w *= 1.0f - c.pos[d];
				p[d] = c.pg[d];
			} else {
				w *= c.pos[d];
				p[d] = min(c.pg[d] + 1u, res - 1u);
			}
			ok = ok && p[d] != 0u && p[d] != res - 1u;
		}
		// (not in the reference: a level without rows, or a row beyond the table, excludes the corner -- a malformed
		// offsets table cannot reach outside the caller's buffers)
		ok = ok && hs != 0u;
		const uint32_t row = ok ? grid_row<D>(p, hs, res) : 0u;
		ok = ok && (long long)row < rows_left;
		c.w[k] = w;
		c.ok[k] = ok;
		c.row[k] = row;
		if (ok) wn += w;
	}
	if (wn == 0.0f) wn = 1e-9f;                  // GC:327-329: (float)(0 + 1e-9)
	c.wn_re = (float)(1.0 / (double)wn);         // GC:330: a double division rounded to fp32 = the fp32 division
}

// The interpolation (GC:337-341) and the reference's dy_dx formula (GC:588-660) from the 2^D corner values `val`
// (excluded corners hold 0: what the dy_dx formula wants, GC:639-642), as functions for mix_grid.hip.  k_grid_fwd keeps the
// same text inline: routed through these two its instruction stream comes out in another order (tools/kernel_hashes.sh),
// and moving code between files is not to change a shipped kernel.
template <int D, int F>
__device__ __forceinline__ Feat<F> interpolate(const Cell<D>& c, const Feat<F> (&val)[1 << D])
{
	Feat<F> out;
#pragma unroll
	for (int ch = 0; ch < F; ch++) out.v[ch] = 0.0f;
#pragma unroll
	for (int k = 0; k < (1 << D); k++) {
		if (!c.ok[k]) continue;
		const float ww = c.w[k] * c.wn_re;
#pragma unroll
		for (int ch = 0; ch < F; ch++) out.v[ch] += ww * val[k].v[ch];   // GC:337-341
	}
	return out;
}

// GC:588-660: for each dimension gd, 2^(D-1) edges along gd; edge idx fixes the other dimensions by its bits
template <int D, int F>
__device__ __forceinline__ void store_dy_dx(const Cell<D>& c, uint32_t res, const Feat<F> (&val)[1 << D], float* dyp)
{
	const float scale = (float)(res - 2u);
#pragma unroll
	for (int gd = 0; gd < D; gd++) {
		Feat<F> rg;
#pragma unroll
		for (int ch = 0; ch < F; ch++) rg.v[ch] = 0.0f;
#pragma unroll
		for (int idx = 0; idx < (1 << (D - 1)); idx++) {
			float w = scale;
			int corner = 0;
#pragma unroll
			for (int nd = 0; nd < D - 1; nd++) {
				const int d = nd >= gd ? nd + 1 : nd;
				if (((idx >> nd) & 1) == 0) {
					w *= 1.0f - c.pos[d];
				} else {
					w *= c.pos[d];
					corner |= 1 << d;
				}
			}
			const Feat<F>& lo = val[corner];
			const Feat<F>& hi = val[corner | (1 << gd)];
#pragma unroll
			for (int ch = 0; ch < F; ch++) rg.v[ch] += w * (hi.v[ch] - lo.v[ch]);   // (* pos_deriv = 1.0f: exact)
		}
		store_feat<F>(dyp + gd * F, rg);
	}
}

// s_l of include/bloomscene_grid.h from the level's max |grad| bits (finite values only) and the point count
__device__ __forceinline__ int grid_scale_exp(uint32_t gbits, int N, int D)
{
	if (gbits == 0u) return 0;
	const uint32_t E = gbits >> 23;
	const int e = E != 0u ? (int)E - 126 : (32 - __clz((int)(gbits & 0x7fffffu))) - 149;
	const int k = (N > 1 ? 32 - __clz((int)(N - 1)) : 0) + D;
	const int s = 61 - k - e;
	return s < 126 ? s : 126;
}

// One contribution v = (w * wn_re) * grad to the element e of a table's fixed-point sums (the header's rule): rounded once
// at the level's scale and added with a 64-bit INTEGER atomic; a non-finite v marks the element instead
__device__ __forceinline__ void grid_contribute(float v, int s, size_t e, unsigned long long* __restrict__ acc,
                                                uint32_t* __restrict__ nonfinite)
{
	if (__builtin_isfinite(v)) {
		const long long q = (long long)__builtin_rintf(__builtin_ldexpf(v, s));
		if (q != 0) atomicAdd(acc + e, (unsigned long long)q);
	} else {
		atomicOr(nonfinite + (e >> 5), 1u << (e & 31));
	}
}

}  // namespace bsr
