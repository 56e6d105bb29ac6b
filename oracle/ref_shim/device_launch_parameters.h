// Forwarding header of the reference-build recipe: threadIdx / blockIdx / blockDim come with the HIP runtime.
#pragma once
#include "cuda_runtime.h"
