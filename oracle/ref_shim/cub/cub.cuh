// Forwarding header of the reference-build recipe: CUB's device-wide primitives are hipCUB's on ROCm.
#pragma once
#include <hipcub/hipcub.hpp>
namespace cub = hipcub;
