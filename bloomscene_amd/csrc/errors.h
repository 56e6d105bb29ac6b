// The calling thread's error string (read back by bsr_last_error) and the two checks every host entry point uses.
// fail() itself is declared in common.h: the units that hold kernels report through it too.  Defined in host_state.hip.
#pragma once
#include "common.h"

namespace bsr {

extern thread_local char g_err[512];   // entry points clear it: g_err[0] = 0

#define HIP_TRY(expr)                                                                              \
	do {                                                                                           \
		hipError_t _e = (expr);                                                                    \
		if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
	} while (0)

// After a launch: always catch launch errors; with debug also synchronise (reference CHECK_CUDA,
// cuda_rasterizer/auxiliary.h:166-173).
#define STAGE_CHECK(name, debug, stream)                                                           \
	do {                                                                                           \
		hipError_t _e = hipGetLastError();                                                         \
		if (_e == hipSuccess && (debug)) _e = hipStreamSynchronize(stream);                        \
		if (_e != hipSuccess) return fail("stage %s failed: %s", name, hipGetErrorString(_e));     \
	} while (0)

}  // namespace bsr
