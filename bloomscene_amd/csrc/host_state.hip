// Host-side state that outlives a call, all of it per thread: the error string, and the pinned landing buffer with the
// deferred overflow check (host_state.h).
#include "../../include/bloomscene_rast.h"
#include "errors.h"
#include "host_state.h"

#include <cstdarg>
#include <cstdio>

namespace bsr {

// ---------------------------------------------------------------- errors
thread_local char g_err[512] = "";

int fail(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return 1;
}

// ---------------------------------------------------------------- host-side cache for the forward's one read-back
SyncCache* sync_cache()
{
	static thread_local SyncCache c;
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { fail("hipGetDevice failed"); return nullptr; }
	if (c.device != dev) {   // first use on this thread, or the thread moved to another GPU
		if (c.copied) (void)hipEventDestroy(c.copied);
		if (c.deferred) (void)hipEventDestroy(c.deferred);
		c.copied = c.deferred = nullptr;
		c.pending = false;
		if (!c.pinned && hipHostMalloc((void**)&c.pinned, 8 * sizeof(int), hipHostMallocMapped) != hipSuccess) {
			c.pinned = nullptr;
			fail("hipHostMalloc failed");
			return nullptr;
		}
		if (hipHostGetDevicePointer((void**)&c.pinned_dev, c.pinned, 0) != hipSuccess) {
			c.pinned_dev = nullptr;
			fail("hipHostGetDevicePointer failed");
			return nullptr;
		}
		if (hipEventCreateWithFlags(&c.copied, hipEventDisableTiming) != hipSuccess ||
		    hipEventCreateWithFlags(&c.deferred, hipEventDisableTiming) != hipSuccess) {
			c.copied = c.deferred = nullptr;
			fail("hipEventCreate failed");
			return nullptr;
		}
		c.device = dev;
		c.last = CallShape{};
	}
	return &c;
}

// One 4-byte device->host read the caller blocks on (selection / visibility counts, anchors.hip): through the calling
// thread's PINNED landing buffer -- an asynchronous copy into pageable memory is staged by the runtime and signals
// later -- and waited for on an event.  Returns 0 on success.
int read_u32_blocking(const uint32_t* dev, uint32_t* out, hipStream_t s)
{
	SyncCache* sc = sync_cache();
	if (!sc) return 1;
	if (hipMemcpyAsync(sc->pinned + 4, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipEventRecord(sc->copied, s) != hipSuccess || hipEventSynchronize(sc->copied) != hipSuccess)
		return fail("reading a count back failed: %s", hipGetErrorString(hipGetLastError()));
	*out = (uint32_t)sc->pinned[4];
	return 0;
}

int check_deferred(SyncCache* sc)
{
	if (!sc->pending) return 0;
	sc->pending = false;
	if (hipEventSynchronize(sc->deferred) != hipSuccess)
		return fail("waiting for the counters of the previous no-readback forward failed: %s", hipGetErrorString(hipGetLastError()));
	const uint32_t kept = (uint32_t)sc->pinned[2];
	sc->nr_shape = sc->pending_shape;
	sc->nr_kept = kept;
	if ((size_t)kept > sc->pending_capacity)
		return fail("the previous BSR_FLAG_NO_READBACK forward of this thread kept %u tile instances but was given a capacity "
		            "of %zu: that frame was not rendered (NaN outputs); its num_rendered was %u",
		            kept, sc->pending_capacity, (uint32_t)sc->pinned[3]);
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

const char* bsr_last_error(void) { return g_err; }

int bsr_check_deferred(void)
{
	g_err[0] = 0;
	SyncCache* sc = sync_cache();
	if (!sc) return 1;
	return check_deferred(sc);
}

}  // extern "C"
