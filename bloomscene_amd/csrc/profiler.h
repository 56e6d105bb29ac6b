// Stage profiler (bench only): a StageTimer around a launch brackets it with an event pair while profiling is on
// (bsr_profile_enable) and does nothing otherwise.  Defined in profiler.hip.
#pragma once
#include "common.h"

namespace bsr {

struct StageRec;
struct StageTimer {
	hipStream_t s;
	StageRec* rec = nullptr;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	StageTimer(const char* name, hipStream_t stream);
	~StageTimer();
};

}  // namespace bsr
