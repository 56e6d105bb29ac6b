// bpow of include/bloomscene_adam.h, written once for the host and the kernel: b^t for t >= 0 by binary exponentiation,
// least significant bit first.  The multiplications, in this order, ARE the definition; there is nothing but fp64
// products here, so no contraction can change the result.
#pragma once

namespace bsr {

__host__ __device__ inline double adam_bpow(double b, long long t)
{
	double r = 1.0, x = b;
	while (t > 0) {
		if (t & 1) r = r * x;
		t >>= 1;
		if (t > 0) x = x * x;
	}
	return r;
}

// ss and bc2s of the header, each formed in fp64 and rounded once
__host__ __device__ inline void adam_step_scalars(double lr, double beta1, double beta2, long long t, float* ss, float* bc2s)
{
	*ss = (float)(lr / (1.0 - adam_bpow(beta1, t)));
	*bc2s = (float)sqrt(1.0 - adam_bpow(beta2, t));
}

}  // namespace bsr
