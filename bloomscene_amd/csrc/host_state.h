// Per-thread host state of the forward: the pinned landing buffer of its one read-back, the size hint for the next
// call's binning scratch, and the deferred overflow check of BSR_FLAG_NO_READBACK forwards.  Defined in host_state.hip.
#pragma once
#include "common.h"

namespace bsr {

// The shape of one forward call: Gaussians, image size, stacked views.
struct CallShape {
	int P = -1, W = -1, H = -1, V = -1;
	bool operator==(const CallShape& o) const { return P == o.P && W == o.W && H == o.H && V == o.V; }
};

// Pinned landing buffer + event for the asynchronous copy of the counters, and the shape / num_rendered
// of the previous forward call on this thread (the size guess of the next one).  Nothing here carries
// results between calls.
struct SyncCache {
	int* pinned = nullptr;       // [4] = flags[0..3] of the forward; [4] = landing word of read_u32_blocking;
	                             // [5] = error flag a prefiltered bsr_visible_filter kernel writes straight into host memory
	int* pinned_dev = nullptr;   // the same buffer as the device addresses it
	hipEvent_t copied = nullptr;
	hipEvent_t deferred = nullptr;   // behind the counters' copy of a BSR_FLAG_NO_READBACK forward (waited for by the NEXT call)
	int device = -1;
	CallShape last;              // the previous forward with a read-back, its (decayed) num_rendered and
	uint32_t last_R = 0;
	uint32_t last_kept = 0;      // kept instances of that call (the hint that picks the next call's binning plan)
	bool pending = false;        // a BSR_FLAG_NO_READBACK forward's copy of the counters is in flight / unchecked
	size_t pending_capacity = 0;
	CallShape pending_shape;     // shape of that forward, and (once its counters have been checked) the shape and kept
	CallShape nr_shape;          // instances of the last checked one: the plan hint of the next no-readback forward
	uint32_t nr_kept = 0;        // of the same shape

	// Whether the binning scratch of a call of this shape can be sized before its count is known, and for how many
	// instances: the previous call's num_rendered + 25 %.
	bool can_guess(const CallShape& now) const { return last == now && last_R > 0; }
	size_t guessed_capacity() const
	{
		const size_t c = (size_t)last_R + (size_t)last_R / 4 + 4096;
		return c > 0x7fffffffu ? 0x7fffffffu : c;
	}
	// size hint for the next call: this call's count, but decaying only by 1/8 per call after a large view
	// (training visits views in random order; a short guess costs a second pass)
	void remember(const CallShape& now, uint32_t R, uint32_t kept)
	{
		const uint32_t decayed = last == now ? last_R - last_R / 8 : 0u;
		last = now;
		last_R = R > decayed ? R : decayed;
		last_kept = kept;
	}
};

// The calling thread's cache, set up for its current device; nullptr (and an error message) if that fails.
SyncCache* sync_cache();

// Deferred overflow check of the calling thread's last BSR_FLAG_NO_READBACK forward (include/bloomscene_rast.h).
int check_deferred(SyncCache* sc);

}  // namespace bsr
