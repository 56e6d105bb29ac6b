// Forwarding header of the reference-build recipe (oracle/reference_build.py): the reference's sources include the
// CUDA runtime by this name; on ROCm it is the HIP runtime.  The runtime API names the reference calls are mapped here,
// so that its sources need no edit for them.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>    // FLT_MAX: the CUDA runtime header drags <cfloat> in, the HIP one does not
#include <cstdint>
#define cudaMalloc hipMalloc
#define cudaFree hipFree
#define cudaMemcpy hipMemcpy
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemcpyHostToDevice hipMemcpyHostToDevice
#define cudaDeviceSynchronize hipDeviceSynchronize
