// A workgroup's dynamic LDS, host side: refuse what the device cannot give one workgroup, and ask for more than the
// default 64 KiB once per kernel and DEVICE (not per call), with the device's whole size.  Two host threads that meet here
// both ask, which is harmless: the state is atomic and both store the same answer.
#pragma once
#include <atomic>
#include "common.h"

namespace bsr {

#define LDS_MAX_DEVICES 64

// the current device and the LDS bytes it gives one workgroup (read once per device)
static int lds_per_workgroup(const char* who, int& dev, int& have)
{
	static std::atomic<int> device_lds[LDS_MAX_DEVICES];   // 0 not asked yet
	if (hipGetDevice(&dev) != hipSuccess || dev < 0) return fail("%s: no current device", who);
	have = dev < LDS_MAX_DEVICES ? device_lds[dev].load(std::memory_order_relaxed) : 0;
	if (have == 0) {
		if (hipDeviceGetAttribute(&have, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || have <= 0)
			return fail("%s: cannot read the device's LDS size", who);
		if (dev < LDS_MAX_DEVICES) device_lds[dev].store(have, std::memory_order_relaxed);
	}
	return 0;
}

// before a launch of Kern with `bytes` of dynamic LDS.  The state is keyed on the kernel itself, not on its type: two
// kernels with one parameter list have one each.
template <auto Kern>
static int reserve_lds(const char* who, size_t bytes)
{
	static std::atomic<int> state[LDS_MAX_DEVICES];   // 0 not asked yet, 1 granted, -1 refused
	int dev = 0, have = 0;
	if (lds_per_workgroup(who, dev, have)) return 1;
	if (bytes > (size_t)have) return fail("%s: a workgroup needs %zu bytes of LDS, the device gives one %d", who, bytes, have);
	if (bytes <= 64 * 1024) return 0;
	const bool tracked = dev < LDS_MAX_DEVICES;
	int st = tracked ? state[dev].load(std::memory_order_relaxed) : 0;
	if (st == 0) {
		st = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, have) == hipSuccess ? 1 : -1;
		if (tracked) state[dev].store(st, std::memory_order_relaxed);
	}
	if (st < 0) return fail("%s: cannot reserve %zu bytes of LDS", who, bytes);
	return 0;
}

}  // namespace bsr
