// Forwarding header of the reference-build recipe: HIP's cooperative groups (this_grid().thread_rank() is all the
// reference uses).
#pragma once
#include <hip/hip_cooperative_groups.h>
