// Forwarding header of the reference-build recipe: torch for ROCm ships its device context under ATen/hip.
#pragma once
#include <ATen/hip/HIPContext.h>
