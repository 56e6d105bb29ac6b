// Stage profiler (bench only): event pairs around the launches of the sampled calls, folded into per-stage totals
// when they are read.  profiler.h declares the StageTimer the host units put around a launch.
#include "../../include/bloomscene_rast.h"
#include "profiler.h"

#include <cstring>
#include <atomic>
#include <mutex>
#include <vector>

namespace bsr {

struct StageRec {
	const char* name;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;   // pending (recorded, not yet read) pairs, oldest first
	size_t head = 0;
	double total_ms = 0;
	int launches = 0;
};
static bool g_prof_on = false;
static int g_prof_every = 1;                      // sample every Nth forward call (and the backward that follows it)
static char g_prof_only[32] = "";                 // non-empty: only this stage is bracketed (bsr_profile_only)
static std::atomic<unsigned> g_prof_calls{0};     // forward calls since enable
static std::atomic<bool> g_prof_this_call{true};  // whether the current forward/backward pair is sampled (process-wide:
                                                  // PyTorch runs the backward on an autograd worker thread)
static std::mutex g_prof_mu;
static std::vector<StageRec> g_stages;
static std::vector<hipEvent_t> g_free_events;   // recycled events (creating thousands of events is slow)

// Fold every pair whose end event has completed into the totals and recycle its events.
// wait == true blocks on unfinished ones (used by bsr_profile_read).
static void drain_stage(StageRec& r, bool wait)
{
	while (r.head < r.ev.size()) {
		auto& p = r.ev[r.head];
		if (wait) {
			if (hipEventSynchronize(p.second) != hipSuccess) break;
		} else if (hipEventQuery(p.second) != hipSuccess) {
			(void)hipGetLastError();   // hipErrorNotReady is not an error
			break;
		}
		float ms = 0;
		if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
			r.total_ms += ms;
			r.launches++;
		}
		g_free_events.push_back(p.first);
		g_free_events.push_back(p.second);
		r.head++;
	}
	if (r.head == r.ev.size()) {
		r.ev.clear();
		r.head = 0;
	}
}

static hipEvent_t take_event()
{
	if (!g_free_events.empty()) {
		hipEvent_t e = g_free_events.back();
		g_free_events.pop_back();
		return e;
	}
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) != hipSuccess) return nullptr;
	return e;
}

StageTimer::StageTimer(const char* name, hipStream_t stream) : s(stream)
{
	if (!g_prof_on) return;
	if (!strcmp(name, "preprocess")) g_prof_this_call = (g_prof_calls.fetch_add(1) % (unsigned)g_prof_every) == 0;
	if (!g_prof_this_call) return;
	if (g_prof_only[0] && strcmp(g_prof_only, name)) return;
	std::lock_guard<std::mutex> lk(g_prof_mu);
	for (auto& r : g_stages)
		if (r.name == name || !strcmp(r.name, name)) rec = &r;
	if (!rec) {
		if (g_stages.size() >= BSR_PROFILE_MAX_STAGES) return;
		g_stages.reserve(BSR_PROFILE_MAX_STAGES);
		g_stages.push_back(StageRec{name});
		rec = &g_stages.back();
	}
	// (pending pairs are folded in by bsr_profile_read / _reset, outside any timed region: reading eight pairs here
	// -- hipEventElapsedTime resolves timestamps on a slow path -- cost one step in 32 of a long bench run 3-4 ms;
	// only a run that never reads keeps the backlog bounded this way)
	if (rec->ev.size() - rec->head >= 4096) drain_stage(*rec, false);
	e0 = take_event();
	e1 = take_event();
	if (!e0 || !e1) { rec = nullptr; return; }
	(void)hipEventRecord(e0, s);
}

StageTimer::~StageTimer()
{
	if (!rec) return;
	(void)hipEventRecord(e1, s);
	std::lock_guard<std::mutex> lk(g_prof_mu);
	rec->ev.emplace_back(e0, e1);
}

}  // namespace bsr

using namespace bsr;

extern "C" {

int bsr_profile_enable(int on)
{
	g_prof_on = on != 0;
	g_prof_every = on > 1 ? on : 1;
	return 0;
}

int bsr_profile_only(const char* stage)
{
	std::lock_guard<std::mutex> lk(g_prof_mu);
	g_prof_only[0] = 0;
	if (stage) {
		strncpy(g_prof_only, stage, sizeof(g_prof_only) - 1);
		g_prof_only[sizeof(g_prof_only) - 1] = 0;
	}
	return 0;
}

int bsr_profile_reset(void)
{
	std::lock_guard<std::mutex> lk(g_prof_mu);
	for (auto& r : g_stages) {
		drain_stage(r, true);
		r.total_ms = 0;
		r.launches = 0;
	}
	return 0;
}

int bsr_profile_read(bsr_stage_profile* out, int max_stages)
{
	std::lock_guard<std::mutex> lk(g_prof_mu);
	int n = 0;
	for (auto& r : g_stages) {
		drain_stage(r, true);
		if (n < max_stages) {
			out[n].name = r.name;
			out[n].total_ms = r.total_ms;
			out[n].launches = r.launches;
			n++;
		}
	}
	return n;
}

}  // extern "C"
