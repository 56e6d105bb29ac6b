// Forwarding header of the reference-build recipe: see cuda_runtime.h.
#pragma once
#include "cuda_runtime.h"
