// The anchor lattice of Quantize_anchor (utils/encodings.py:215-227), rule A of include/bloomscene_anchor_state.h, written
// once for the two units that need it: anchor_state.hip (the quantised anchors of a training iteration) and
// anchor_codec.hip (the lattice indices the position coder writes, and the anchors its decoder returns).  The decoder's
// anchors are get_anchor's bit for bit because both go through anchor_dequantise.
#pragma once
#include "common.h"

namespace bsr {

// torch.div(a, b, rounding_mode='floor') on fp32, operation for operation (the header writes it out)
__device__ __forceinline__ float floor_div(float a, float b)
{
	if (b == 0.0f) return a / b;
	const float mod = fmodf(a, b);
	float div = (a - mod) / b;
	if (mod != 0.0f && (b < 0.0f) != (mod < 0.0f)) div = div - 1.0f;
	if (div != 0.0f) {
		float q = floorf(div);
		if (div - q > 0.5f) q = q + 1.0f;
		return q;
	}
	return copysignf(0.0f, a / b);
}

__device__ __forceinline__ float anchor_interval(float lo, float hi) { return ((hi - lo) * (float)(1.0 / 65535.0)) + 1e-6f; }

// the lattice index of x as a float in [0, 65535] (a NaN stays a NaN)
__device__ __forceinline__ float anchor_lattice_index(float x, float lo, float interval)
{
	const float q = floor_div(x - lo, interval);
	return q < 0.0f ? 0.0f : (q > 65535.0f ? 65535.0f : q);
}

__device__ __forceinline__ float anchor_dequantise(float q, float lo, float interval) { return q * interval + lo; }

__device__ __forceinline__ float quantize_anchor(float x, float lo, float hi)
{
	const float interval = anchor_interval(lo, hi);
	return anchor_dequantise(anchor_lattice_index(x, lo, interval), lo, interval);
}

}  // namespace bsr
