// Forwarding header of the reference-build recipe: half types of the HIP runtime.
// CUDA declares atomicAdd(__half2*, __half2); ROCm's hip_fp16.h has the operation under the name unsafeAtomicAdd only.
// The reference's half instantiations need the CUDA name to compile; the fp32 tests never reach them.
#pragma once
#include <hip/hip_fp16.h>
__device__ inline __half2 atomicAdd(__half2* address, __half2 value) { return unsafeAtomicAdd(address, value); }
