// Forwarding header of the reference-build recipe: the reference includes this header and uses nothing of it.
#pragma once
#include "../cooperative_groups.h"
