// The two device steps of BloomScene's anchor densification for gfx950 (include/bloomscene_densify.h):
// GaussianModel.anchor_growing, scene/gaussian_model.py:807-895 ("GM").
//
// bsr_scatter_max (torch_scatter.scatter_max of GM:862, and the repeat of GM:861 through row_map):
//   k_densify_fill          arg[G * F] = 0, the packed value of "no contribution"
//   k_scatter_max_pack      one thread per (e, f): atomic 64-bit unsigned maximum of
//                               key(src[r(e), f]) << 32 | (0xffffffff - e)
//                           into arg[index(e, f), f].  key is monotone in the header's order (NaN -> 0xffffffff, -0 -> the
//                           key of +0, negative values -> ~bits, others -> bits | 0x80000000) and at least 0x007fffff (-inf),
//                           so no contribution packs to 0; among equal keys the smaller e packs higher.
//   k_scatter_max_unpack    one thread per (g, f): 0 -> (+0.0, E); else e from the low word, out = the bits of src[r(e), f]
//                           read again (the key has lost the sign of a zero and a NaN's payload), arg = e -- in place.
// WHY IT IS DETERMINISTIC.  The packed words of one (g, f) are distinct (e is in the low word), an unsigned maximum does
// not depend on the order of its operands, and nothing else is accumulated: the winner is the header's, whatever the
// schedule.  No float atomics.
//
// bsr_voxel_isin (GM:838-849): an open-addressing table of key ROW NUMBERS in the scratch, 2^k >= 2 N slots.
//   k_densify_fill          every slot = 0xffffffff (empty)
//   k_voxel_insert          one thread per key row: probe linearly from hash(row); claim an empty slot with an integer
//                           compare-and-swap, or stop at a slot whose row equals this one in all three components
//   k_voxel_lookup          one thread per query: probe from hash(query) until a slot's row equals it (1) or the slot is
//                           empty (0)
// The load is at most 1/2, so there is always an empty slot and every probe ends (the loops are bounded by the table
// size all the same).  A slot only ever changes from empty to a row number, and a key row is input: a reader that
// sees a row number may read that row.  After k_voxel_insert every distinct key row owns exactly one slot on its probe
// path with no empty slot before it -- which of its duplicates got there first decides the number in the slot, not the
// set of rows in the table, and the mask is a property of that set.
#include "common.h"
#include "../../include/bloomscene_densify.h"

namespace bsr {

#define BSR_DENSIFY_BLOCK 256
#define BSR_DENSIFY_MAX_BLOCKS (1 << 18)   // grid-stride beyond 2^26 elements
#define BSR_VOXEL_EMPTY 0xffffffffu

template <typename T>
__global__ void __launch_bounds__(BSR_DENSIFY_BLOCK) k_densify_fill(T* __restrict__ p, size_t n, T value)
{
	for (size_t i = (size_t)blockIdx.x * BSR_DENSIFY_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BSR_DENSIFY_BLOCK)
		p[i] = value;
}

static unsigned blocks_for(size_t n)
{
	const size_t nb = (n + BSR_DENSIFY_BLOCK - 1) / BSR_DENSIFY_BLOCK;
	return (unsigned)(nb < BSR_DENSIFY_MAX_BLOCKS ? nb : BSR_DENSIFY_MAX_BLOCKS);
}

// ---- scatter_max ----

// monotone in the header's order of values; >= 0x007fffff
__device__ __forceinline__ uint32_t scatter_order_key(uint32_t bits)
{
	if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;   // NaN: above everything, all equal
	if (bits == 0x80000000u) bits = 0u;                            // -0 == +0
	return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// I: the type the element number is divided in (uint32_t while E * F fits)
template <typename I>
__global__ void __launch_bounds__(BSR_DENSIFY_BLOCK) k_scatter_max_pack(size_t total, int S, int F, int G,
                                                                        const float* __restrict__ src,
                                                                        const long long* __restrict__ row_map,
                                                                        const long long* __restrict__ index,
                                                                        long long is0, long long is1,
                                                                        unsigned long long* __restrict__ packed)
{
	for (size_t t = (size_t)blockIdx.x * BSR_DENSIFY_BLOCK + threadIdx.x; t < total;
	     t += (size_t)gridDim.x * BSR_DENSIFY_BLOCK) {
		const I e = (I)t / (I)F;
		const I f = (I)t - e * (I)F;
		const long long g = index[(long long)e * is0 + (long long)f * is1];
		if (g < 0 || g >= (long long)G) continue;
		long long r = (long long)e;
		if (row_map) {
			r = row_map[e];
			if (r < 0 || r >= (long long)S) continue;
		}
		const uint32_t bits = __float_as_uint(src[(size_t)r * F + f]);
		const unsigned long long v = ((unsigned long long)scatter_order_key(bits) << 32) |
		                             (unsigned long long)(0xffffffffu - (uint32_t)e);
		atomicMax(&packed[(size_t)g * F + f], v);
	}
}

__global__ void __launch_bounds__(BSR_DENSIFY_BLOCK) k_scatter_max_unpack(int n, int E, int F, const float* __restrict__ src,
                                                                          const long long* __restrict__ row_map,
                                                                          float* __restrict__ out, long long* arg)
{
	const size_t t = (size_t)blockIdx.x * BSR_DENSIFY_BLOCK + threadIdx.x;
	if (t >= (size_t)n) return;
	const unsigned long long p = (unsigned long long)arg[t];
	float o = 0.0f;
	long long a = (long long)E;
	if (p != 0ull) {
		const uint32_t e = 0xffffffffu - (uint32_t)p;
		if (e < (uint32_t)E) {   // (always true; a guard against a broken word)
			const size_t r = row_map ? (size_t)row_map[e] : (size_t)e;   // (in range: it was when e contributed)
			o = src[r * F + (size_t)((uint32_t)t % (uint32_t)F)];
			a = (long long)e;
		}
	}
	out[t] = o;
	arg[t] = a;
}

// ---- voxel membership ----

__device__ __forceinline__ uint32_t voxel_fmix(uint32_t h)   // (the finaliser of MurmurHash3: a bijection of 32 bits)
{
	h ^= h >> 16; h *= 0x85ebca6bu;
	h ^= h >> 13; h *= 0xc2b2ae35u;
	h ^= h >> 16;
	return h;
}
// every component goes through a full mix before the next is added: lattices (x == y == z, multiples of 2^16) spread
__device__ __forceinline__ uint32_t voxel_hash(int x, int y, int z)
{
	uint32_t h = voxel_fmix((uint32_t)x + 0x9e3779b9u);
	h = voxel_fmix(h + (uint32_t)y + 0x9e3779b9u);
	h = voxel_fmix(h + (uint32_t)z + 0x9e3779b9u);
	return h;
}

__global__ void __launch_bounds__(BSR_DENSIFY_BLOCK) k_voxel_insert(int N, const int* __restrict__ keys, uint32_t slots_mask,
                                                                    uint32_t* table)
{
	const size_t i = (size_t)blockIdx.x * BSR_DENSIFY_BLOCK + threadIdx.x;
	if (i >= (size_t)N) return;
	const int x = keys[3 * i], y = keys[3 * i + 1], z = keys[3 * i + 2];
	uint32_t h = voxel_hash(x, y, z) & slots_mask;
	for (uint32_t probes = 0; probes <= slots_mask; probes++) {
		// (a slot only ever goes from empty to a row number: a stale read can only send a taken slot to the swap)
		uint32_t seen = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (seen == BSR_VOXEL_EMPTY) seen = atomicCAS(&table[h], BSR_VOXEL_EMPTY, (uint32_t)i);
		if (seen == BSR_VOXEL_EMPTY) return;   // claimed
		if (seen < (uint32_t)N && keys[3 * (size_t)seen] == x && keys[3 * (size_t)seen + 1] == y &&
		    keys[3 * (size_t)seen + 2] == z)
			return;                            // this row is in the table already
		h = (h + 1u) & slots_mask;
	}
}

__global__ void __launch_bounds__(BSR_DENSIFY_BLOCK) k_voxel_lookup(int U, int N, const int* __restrict__ query,
                                                                    const int* __restrict__ keys, uint32_t slots_mask,
                                                                    const uint32_t* __restrict__ table,
                                                                    unsigned char* __restrict__ mask)
{
	const size_t u = (size_t)blockIdx.x * BSR_DENSIFY_BLOCK + threadIdx.x;
	if (u >= (size_t)U) return;
	const int x = query[3 * u], y = query[3 * u + 1], z = query[3 * u + 2];
	uint32_t h = voxel_hash(x, y, z) & slots_mask;
	unsigned char found = 0;
	for (uint32_t probes = 0; probes <= slots_mask; probes++) {
		const uint32_t row = table[h];
		if (row >= (uint32_t)N) break;   // empty (or not a row number: never dereferenced)
		if (keys[3 * (size_t)row] == x && keys[3 * (size_t)row + 1] == y && keys[3 * (size_t)row + 2] == z) {
			found = 1;
			break;
		}
		h = (h + 1u) & slots_mask;
	}
	mask[u] = found;
}

// slots of the table: the power of two >= max(2 N, 64)
static size_t voxel_slots(size_t N)
{
	size_t s = 64;
	while (s < 2 * N) s <<= 1;
	return s;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

int bsr_scatter_max(int E, int S, int F, int G, const float* src, const long long* row_map, const long long* index,
                    long long is0, long long is1, float* out, long long* arg, void* stream)
{
	const char* who = "bsr_scatter_max";
	if (E < 0 || S < 0 || F < 1 || G < 0) return fail("%s: need E >= 0, S >= 0, F >= 1, G >= 0 (got %d, %d, %d, %d)", who, E, S, F, G);
	if ((long long)G * F > 0x7fffffffLL) return fail("%s: G * F must be below 2^31 (got %d * %d)", who, G, F);
	if (!row_map && S != E) return fail("%s: without row_map S must equal E (got %d, %d)", who, S, E);
	if (is0 < 0 || is1 < 0) return fail("%s: index strides must be >= 0 (got %lld, %lld)", who, is0, is1);
	if (G == 0) return 0;
	if (!out || !arg) return fail("%s: NULL output", who);
	if (((uintptr_t)out & 3) || ((uintptr_t)arg & 7)) return fail("%s: out must be 4-byte and arg 8-byte aligned", who);
	if (E > 0 && (!src || !index)) return fail("%s: NULL input", who);
	if (((uintptr_t)src & 3) || (((uintptr_t)index | (uintptr_t)row_map) & 7))
		return fail("%s: src must be 4-byte, index and row_map 8-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const dim3 blk(BSR_DENSIFY_BLOCK);
	const size_t n = (size_t)G * F, total = (size_t)E * F;
	unsigned long long* packed = (unsigned long long*)arg;
	hipLaunchKernelGGL(k_densify_fill<unsigned long long>, dim3(blocks_for(n)), blk, 0, st, packed, n, 0ull);
	if (total > 0) {
		if (total <= 0xffffffffull)
			hipLaunchKernelGGL(k_scatter_max_pack<uint32_t>, dim3(blocks_for(total)), blk, 0, st, total, S, F, G, src,
			                   row_map, index, is0, is1, packed);
		else
			hipLaunchKernelGGL(k_scatter_max_pack<uint64_t>, dim3(blocks_for(total)), blk, 0, st, total, S, F, G, src,
			                   row_map, index, is0, is1, packed);
	}
	hipLaunchKernelGGL(k_scatter_max_unpack, dim3((unsigned)((n + BSR_DENSIFY_BLOCK - 1) / BSR_DENSIFY_BLOCK)), blk, 0, st,
	                   (int)n, E, F, src, row_map, out, arg);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

size_t bsr_voxel_isin_scratch_bytes(int N)
{
	if (N <= 0 || N > BSR_VOXEL_MAX_KEYS) return 0;
	return align_up(voxel_slots((size_t)N) * 4, 256);
}

int bsr_voxel_isin(int U, int N, const int* query, const int* keys, unsigned char* mask, void* scratch, void* stream)
{
	const char* who = "bsr_voxel_isin";
	if (U < 0 || N < 0 || N > BSR_VOXEL_MAX_KEYS) return fail("%s: need U >= 0 and 0 <= N <= %d (got %d, %d)", who, BSR_VOXEL_MAX_KEYS, U, N);
	if (U == 0) return 0;
	if (!query || !mask) return fail("%s: NULL buffer", who);
	if ((uintptr_t)query & 3) return fail("%s: query must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const dim3 blk(BSR_DENSIFY_BLOCK);
	if (N == 0) {
		hipLaunchKernelGGL(k_densify_fill<unsigned char>, dim3(blocks_for((size_t)U)), blk, 0, st, mask, (size_t)U,
		                   (unsigned char)0);
	} else {
		if (!keys || !scratch) return fail("%s: NULL buffer", who);
		if (((uintptr_t)keys | (uintptr_t)scratch) & 3) return fail("%s: keys and scratch must be 4-byte aligned", who);
		const size_t slots = voxel_slots((size_t)N);
		uint32_t* table = (uint32_t*)scratch;
		hipLaunchKernelGGL(k_densify_fill<uint32_t>, dim3(blocks_for(slots)), blk, 0, st, table, slots, BSR_VOXEL_EMPTY);
		hipLaunchKernelGGL(k_voxel_insert, dim3((unsigned)(((size_t)N + BSR_DENSIFY_BLOCK - 1) / BSR_DENSIFY_BLOCK)), blk, 0,
		                   st, N, keys, (uint32_t)(slots - 1), table);
		hipLaunchKernelGGL(k_voxel_lookup, dim3((unsigned)(((size_t)U + BSR_DENSIFY_BLOCK - 1) / BSR_DENSIFY_BLOCK)), blk, 0,
		                   st, U, N, query, (const int*)keys, (uint32_t)(slots - 1), (const uint32_t*)table, mask);
	}
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
