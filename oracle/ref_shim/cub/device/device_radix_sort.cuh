// Forwarding header of the reference-build recipe: see cub/cub.cuh.
#pragma once
#include "../cub.cuh"
