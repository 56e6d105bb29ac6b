// Per-tile depth sort: the kernels (primitives: tile_sort.h) and their launches.
//
//   5. (binning.hip: steps 1-4) every segment is sorted by its 64-bit key (depth bits, Gaussian id) in LDS:
//      k_sort_tiles_tiny / small / mid / wide by size class, behind either placement pass of binning.hip,
//   6. frames of up to 8192 tiles with at most BSR_BKT_BIG_PER_TILE kept instances per tile (binning.hip: binning_plan)
//      take steps 3-5 in ONE launch (k_bucket_sort: the tile segments laid out inside their pass-1 bucket).
#include "tile_sort.h"
#include "launch.h"

namespace bsr {

// Tiny class (n <= 64: every tile of a sparse camera-sweep view): one wave per tile, one key per lane, no LDS and no
// synchronisation at all -- a key's place is the number of smaller keys ((depth bits, id) pairs are unique within a
// tile), counted against the wave's keys broadcast one by one from SGPRs.  27 keys: ~110 instructions, against a
// merge network that keeps 4 of 64 lanes busy and a 32-KB LDS footprint that caps the small class at 20 waves per CU.
__global__ void __launch_bounds__(256) k_sort_tiles_tiny(int T, const int* __restrict__ n_ptr, int capacity,
                                                         const uint2* __restrict__ tile_range,
                                                         const BinElem* __restrict__ elems,
                                                         uint32_t* __restrict__ point_list, int compact)
{
	const int lane = threadIdx.x & 63;
	const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (tile >= T) return;
	const int n_instances = *n_ptr;
	const uint2 range = tile_range[tile];
	const uint32_t start = range.x;
	const int n = (int)(range.y - range.x);
	if (n_instances > capacity || n > 64 || n <= 0) return;   // (scratch too small: stage is re-run) / another class / empty
	uint64_t key = ~0ull;
	if (lane < n) key = elem_key_m(elems, (size_t)start + (size_t)lane, compact);
	const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
	uint32_t rank = 0;
	for (int j = 0; j < n; j++) {
		const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, j) << 32) |
		                    (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)lo, j);
		rank += kj < key ? 1u : 0u;
	}
	if (lane < n) point_list[start + rank] = lo;
}

// Small class (min_n < n <= BSR_SORT_SMALL): one WAVE per tile, four tiles per workgroup, no workgroup barrier; 8 keys per
// lane and round (16 in two trips beyond 512 keys).
__global__ void __launch_bounds__(256) k_sort_tiles_small(int T, const int* __restrict__ n_ptr, int capacity,
                                                          const uint2* __restrict__ tile_range,
                                                          const BinElem* __restrict__ elems,
                                                          uint32_t* __restrict__ point_list, int sort_mode, int min_n,
                                                          int compact)
{
	__shared__ uint64_t s_keys[4][BSR_SORT_SMALL];
	__shared__ uint32_t s_rank[4][512];   // rank_sort's counters: up to 1024 buckets per wave
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int tile = blockIdx.x * 4 + wave;
	if (tile >= T || *n_ptr > capacity) return;   // (more instances than the scratch was sized for: stage is re-run)
	const uint2 range = tile_range[tile];
	const uint32_t start = range.x;
	const int n = (int)(range.y - range.x);
	if (n > BSR_SORT_SMALL || n <= min_n) return;   // on the big-tile list / sorted by k_sort_tiles_tiny (min_n = 64) or empty
	// bucket-and-rank sort first (sort_mode 0); a segment it declines -- depths piled on one value -- goes to the network
	if (sort_mode == 0 && n > 64) {
		if (n <= 512) {
			if (rank_sort_from<64, 8, 9, false>(ElemKeys{elems, compact}, n, lane, s_keys[wave], s_rank[wave], nullptr, start, point_list)) return;
		} else {
			if (rank_sort_from<64, 16, 10, false>(ElemKeys{elems, compact}, n, lane, s_keys[wave], s_rank[wave], nullptr, start, point_list)) return;
		}
		round_sync<false>();
	}
	int n2 = 8;
	while (n2 < n) n2 <<= 1;
	sort_segment_wave<3>(s_keys[wave], n2, start, n, lane, elems, point_list, (sort_mode & 1) != 0, compact);   // (> 512 keys: two runs per lane)
}

// Wide classes, ONE launch (a frame without long lists -- C3 -- pays one near-empty launch instead of two; until round 5
// the two upper classes had a 1024-thread, 64-KB kernel of their own): 512 threads, 4096 keys = 32 KB of LDS.
// Workgroups [0, g1) stride over the (1024, 4096] list (big_tiles[0..T), count flags[1]) and sort each segment in LDS;
// workgroups [g1, g1 + gw) stride over the two longer lists (big_tiles[T..2T), flags[4]; [2T..3T), flags[5]) with the
// hybrid: every 4096-key chunk sorted in LDS, the merge steps between chunks in global scratch (`keys` = the free
// ping-pong buffer viewed as u64), the steps inside a chunk in LDS again.  Bounded grids: n instances fill at most
// n / 1025 (n / 4097) such tiles, capped -- the workgroups stride.
#define BSR_SORT_NT 512
// (64 VGPRs: with 33 KB of LDS a CU holds four workgroups = 8 waves per SIMD; the hybrid path alone would take 70 and
// cost the common (1024, 4096] class its fourth workgroup: C5's tile sort 0.184 -> 0.206 ms)
#ifndef BSR_WIDE_WAVES
#define BSR_WIDE_WAVES 6
#endif
// The lower half of the first wide class, (1024, 2048] keys, in a launch of its own (round 6): 256 threads, 16 KB of keys +
// 2 KB of counters.  A segment's sort is short (~3 us); what a workgroup of k_sort_tiles_wide spends per segment is
// mostly the chain of dependent loads ahead of it (list entry -> range -> keys) and the drain of its stores behind it.
// Here the workgroups are few enough to be resident all at once and stride over the work list (big_tiles[0..flags[1]))
// with the loads of the NEXT segments in flight under the sort of the current one: the range two entries ahead, the keys
// (8 per thread, in registers) one entry ahead.  k_sort_tiles_wide skips what is sorted here.
#ifndef BSR_SORT_MID_WGS
#define BSR_SORT_MID_WGS 1280   // five workgroups per CU
#endif
#ifndef BSR_MID_NBLOG
#define BSR_MID_NBLOG 11   // 2048 buckets for up to 2048 keys (1024: +2 us on the dense leg)
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) k_sort_tiles_mid(int g1, const int* __restrict__ n_ptr, int capacity,
                                                                 const uint2* __restrict__ tile_range,
                                                                 const uint32_t* __restrict__ big_tiles,
                                                                 const int* __restrict__ flags,
                                                                 const BinElem* __restrict__ elems,
                                                                 uint32_t* __restrict__ point_list, int sort_mode, int compact)
{
	__shared__ uint64_t s_keys[BSR_SORT_MID];
	__shared__ uint32_t s_rank[(1 << BSR_MID_NBLOG) / 2 + 16];   // rank_sort's counters + its reduction words
	const int tid = threadIdx.x;
	if (*n_ptr > capacity) return;
	const ElemKeys src{elems, compact};
	const int count = flags[1];
	// the segment of list entry b if it belongs to this class, else an empty one
	auto segment = [&](int b) {
		if (b >= count) return make_uint2(0u, 0u);
		const uint2 r = tile_range[big_tiles[b]];
		const int n = (int)(r.y - r.x);
		return (n > BSR_SORT_SMALL && n <= BSR_SORT_MID) ? r : make_uint2(0u, 0u);
	};
	auto load_keys = [&](const uint2 r, uint64_t (&e)[8]) {
		const int n = (int)(r.y - r.x);
#pragma unroll
		for (int q = 0; q < 8; q++) e[q] = tid + 256 * q < n ? src((size_t)r.x + (size_t)(tid + 256 * q)) : 0ull;
	};
	uint2 cur = segment((int)blockIdx.x), nxt = segment((int)blockIdx.x + g1);
	uint64_t e[8];
	load_keys(cur, e);
	for (int b = blockIdx.x; b < count; b += g1) {
		const uint2 nxt2 = segment(b + 2 * g1);
		uint64_t en[8];
		load_keys(nxt, en);
		const int n = (int)(cur.y - cur.x);
		if (n > 0) {   // (uniform over the workgroup)
			bool done = false;
			if (sort_mode == 0) {   // bucket-and-rank sort; a declined segment goes through the network (which loads it again)
				done = rank_sort<256, 8, BSR_MID_NBLOG, true>(e, n, tid, s_keys, s_rank, s_rank + (1 << BSR_MID_NBLOG) / 2, cur.x, point_list);
				__syncthreads();
			}
			if (!done) {
				sort_segment_block<256, 3>(s_keys, BSR_SORT_MID, cur.x, n, tid, src, point_list, (sort_mode & 1) != 0);
				__syncthreads();
			}
		}
		cur = nxt;
		nxt = nxt2;
#pragma unroll
		for (int q = 0; q < 8; q++) e[q] = en[q];
	}
}

__global__ void __launch_bounds__(BSR_SORT_NT) __attribute__((amdgpu_waves_per_eu(BSR_WIDE_WAVES, 8))) k_sort_tiles_wide(int T, int g1, const int* __restrict__ n_ptr, int capacity,
                                                                 const uint2* __restrict__ tile_range,
                                                                 const uint32_t* __restrict__ big_tiles,
                                                                 const int* __restrict__ flags,
                                                                 const BinElem* __restrict__ elems, uint64_t* keys,
                                                                 uint32_t* __restrict__ point_list, int sort_mode, int compact,
                                                                 int lds_min)   // segments of up to lds_min keys: another kernel's
{
	constexpr int NT = BSR_SORT_NT, CH = BSR_SORT_CHUNK;
	__shared__ uint64_t s_keys[CH];
	__shared__ uint32_t s_rank[1024 + 32];   // rank_sort's counters (2048 buckets) + its reduction words
	const int tid = threadIdx.x;
	if (*n_ptr > capacity) return;
	const ElemKeys src{elems, compact};
	if ((int)blockIdx.x < g1) {
		const int count = flags[1];
		for (int b = blockIdx.x; b < count; b += g1) {
			const uint32_t tile = big_tiles[b];
			const uint2 range = tile_range[tile];
			const uint32_t start = range.x;
			const int n = (int)(range.y - range.x);
			if (n <= lds_min || n > CH) continue;   // another class (uniform over the workgroup)
			sort_long_tile_lds<NT>(s_keys, s_rank, start, n, tid, src, point_list, sort_mode);
		}
		return;
	}
	const int gw = (int)gridDim.x - g1, count4 = flags[4], count8 = flags[5];
	for (int b = (int)blockIdx.x - g1; b < count4 + count8; b += gw) {
		const uint32_t tile = b < count4 ? big_tiles[(size_t)T + b] : big_tiles[2 * (size_t)T + (b - count4)];
		const uint2 range = tile_range[tile];
		const uint32_t start = range.x;
		const int n = (int)(range.y - range.x);
		if (n <= CH) continue;
		sort_long_tile_hybrid<NT>(s_keys, keys + start, start, n, tid, src, point_list);
	}
}

// ---- bucket-owned second pass + per-tile sort, ONE launch (frames of up to 8192 tiles with short lists) ----------------
// After pass 1 (k_emit_scatter) the instances of tile t all lie in bucket t & 255, a contiguous range whose bounds follow
// from the 256 digit totals alone.  Nothing downstream needs the tile segments in TILE order -- the tile walks and the
// backward take (start, end) per tile from tile_range -- so the segments of a bucket's tiles can simply be laid out
// inside the bucket's own range: a segment's position then depends on the counts of ITS bucket only, and the chain
// k_tile_count -> k_tile_starts (one workgroup, a global scan) -> k_tile_scatter -> k_sort_tiles_small ->
// k_sort_tiles_wide  (five launches, the elements written and read once more) collapses into one kernel without any
// communication between workgroups:
//   workgroup (bucket d, part j of k = 2^k_log2): owns the bucket's tiles whose high byte hi = j (mod k) -- at most
//   NW * TPW of them, tile L = hi / k in LDS area L -- and streams the WHOLE bucket once (8-byte elements; the k parts
//   of a bucket run on one XCD back to back: one HBM read, k - 1 L2 hits).  An element of one of its tiles takes its
//   slot in the tile's area from an LDS counter (= the tile's count in the end); of the others only those of EARLIER
//   parts are counted (one wave ballot per element, no LDS traffic), which is all the layout needs: the bucket's range
//   holds part 0's tiles, then part 1's, ..., inside a part in order of L -- part j begins behind the elements of the
//   parts before it, which every workgroup of the bucket counts alike, so the segments tile the range.
//   Then the ranges are written and every wave sorts its TPW tiles in place (rank_sort, or the wave-owned network of
//   k_sort_tiles_small, from LDS instead of global memory; up to 64 keys: ranks by counting) and writes the ids.
//   A tile of more than AREA instances (rare where this kernel is chosen) is staged as plain keys in global scratch
//   by a second pass over the bucket and sorted by the whole workgroup with the long-tile routines above.
// Chosen by the host from sizes alone (binning_plan): both this kernel and the chain are correct for every input.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_bucket_sort<2048, 1> needs 144 KB of static LDS: this unit is written for gfx950 (160 KB per workgroup) only"
#endif
#define BSR_BKT_NT 512
#define BSR_BKT_NW (BSR_BKT_NT / 64)
typedef uint32_t bsr_u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
template <int AREA, int TPW>   // keys per tile area (512 / 1024 / 2048); tiles per wave
__global__ void __launch_bounds__(BSR_BKT_NT) k_bucket_sort(int T, int k_log2, const int* __restrict__ n_ptr, int capacity,
                                                            const uint32_t* __restrict__ digit_total1,
                                                            const BinElem* __restrict__ elems, uint2* __restrict__ tile_range,
                                                            uint64_t* big_keys, uint32_t* __restrict__ point_list,
                                                            int sort_mode)
{
	const int force_int = sort_mode & 1;
	constexpr int NT = BSR_BKT_NT, NW = BSR_BKT_NW, NA = NW * TPW;
	// TPW = 2: a wave sorts its two tiles side by side, one per 32-lane half, 16 keys per lane and round (slots swz_m<4>);
	// TPW = 1: one tile per wave, 8 keys per lane and round (slots swz_m<3>)
	constexpr int SM = TPW == 2 ? 4 : 3;
	static_assert(TPW == 1 || (TPW == 2 && AREA == 512), "paired sort: two 512-key areas per wave");
	static_assert(NA * AREA >= BSR_SORT_CHUNK, "the long-tile routines sort 4096-key chunks in this LDS");
	__shared__ uint64_t s_keys[NA * AREA];          // one area per owned tile; the long-tile routines use the first 4096 slots
	__shared__ uint32_t s_cnt[NA];                  // elements per owned tile (the fill counters of the pass)
	__shared__ uint32_t s_part[4];                  // [0]: elements of the bucket in earlier parts
	__shared__ uint32_t s_cur[NA];                  // second pass: fill counters of this part's long tiles
	// rank_sort's counters: 512 buckets per wave, 1024 where an area holds 2048 keys (the long-tile routine: all of it)
	constexpr int RNBLOG = AREA > 1024 ? 10 : 9, RDW = (1 << RNBLOG) / 2;
	__shared__ uint32_t s_rank[NW][RDW];
	static_assert(NW * RDW >= 1024 + 32, "sort_long_tile_lds takes 2048 buckets + its reduction words");
	static_assert(sizeof(s_keys) + sizeof(s_cnt) + sizeof(s_part) + sizeof(s_cur) + sizeof(s_rank) <= 160 * 1024,
	              "static LDS beyond gfx950's 160 KB per workgroup");
	const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int k = 1 << k_log2;                      // 1, 2 or 4
	// parts of one bucket are neighbours on one XCD: workgroups b, b + 8, b + 16, ... share an XCD
	const int xcd = (int)blockIdx.x & 7, r = (int)blockIdx.x >> 3;
	const int j = r & (k - 1), d = ((r >> k_log2) << 3) | xcd;
	const int nt = d < T ? ((T - 1 - d) >> BSR_RADIX_BITS) + 1 : 0;      // tiles of this bucket: (hi << 8) | d < T
	const int m = nt > j ? (nt - j + k - 1) >> k_log2 : 0;               // ... of this part: hi = j + k L, L < m <= NA
	const int n_all = *n_ptr;
	if (n_all > capacity) return;   // scratch too small: the stage is re-run
	if (n_all <= 0) {               // nothing kept: every tile is empty
		if (tid < m) tile_range[(uint32_t)((j + (tid << k_log2)) << BSR_RADIX_BITS) | (uint32_t)d] = make_uint2(0u, 0u);
		return;
	}
	// the bucket's range: its base among the 256 digits (written by k_emit_scatter behind the totals) and its total
	if (tid < NA) s_cnt[tid] = 0u;
	if (tid < 4) s_part[tid] = 0u;
	__syncthreads();
	const uint32_t beg = digit_total1[BSR_RADIX_BINS + d], size = digit_total1[d];   // (uniform: scalar loads)
	const uint2* const src = reinterpret_cast<const uint2*>(elems) + beg;
	// An element of the pass is counted if it belongs to an EARLIER part (all the layout needs of the other parts: where
	// this part's tiles begin -- one vote per element; until the 2048-key areas every part was counted, k votes); if it
	// belongs to a tile of this part it takes its slot in the tile's area from the tile's LDS counter.  Eight elements at
	// a time: first all eight returning atomics, then the eight stores -- element by element every atomic's round trip
	// through the LDS was waited for before the next element was looked at (16 round trips per trip of a wave).
	uint32_t before = 0u;   // (wave-uniform: a scalar register)
	auto take8 = [&](const bool full, const uint32_t i, const bsr_u32x4_a8 (&v)[8], const int u0) {
		uint32_t pos[8];
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const bsr_u32x4_a8 q = v[u0 + (e >> 1)];
			const uint32_t w0 = (e & 1) ? q.z : q.x;
			const uint32_t ie = i + 2u * (uint32_t)((e >> 1) * NT) + (uint32_t)(e & 1);
			const bool valid = full || ie < size;
			const uint32_t hi = w0 >> 24;
			const uint32_t part = hi & (uint32_t)(k - 1);
			if (j > 0) {   // (j: workgroup-uniform.  Two votes AND-ed on the scalar side: a vote on `valid && ...` is a mask
				           // materialised in a VGPR and compared again)
				const uint64_t m = wave_ballot(part < (uint32_t)j);
				before += (uint32_t)__popcll(full ? m : (m & wave_ballot(valid)));
			}
			pos[e] = 0xffffffffu;
			if (valid && (int)part == j) pos[e] = atomicAdd(&s_cnt[hi >> k_log2], 1u);   // LDS
		}
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const bsr_u32x4_a8 q = v[u0 + (e >> 1)];
			const uint32_t w0 = (e & 1) ? q.z : q.x, w1 = (e & 1) ? q.w : q.y;
			if (pos[e] < (uint32_t)AREA)
				s_keys[(w0 >> (24 + k_log2)) * AREA + swz_m<SM>((int)pos[e])] = ((uint64_t)w1 << 32) | (uint64_t)(w0 & 0x00ffffffu);
		}
	};
	// ---- the pass over the bucket: two elements per 16-byte load, eight loads in flight
	auto request = [&](uint32_t i0, bsr_u32x4_a8 (&v)[8]) {
#pragma unroll
		for (int u = 0; u < 8; u++) {
			const uint32_t i = i0 + 2u * (uint32_t)(u * NT + tid);
			if (i + 1 < size) v[u] = *reinterpret_cast<const bsr_u32x4_a8*>(src + i);
			else if (i < size) { const uint2 e = src[i]; v[u] = bsr_u32x4_a8{e.x, e.y, 0u, 0u}; }
			else v[u] = bsr_u32x4_a8{0u, 0u, 0u, 0u};
		}
	};
	auto consume = [&](uint32_t i0, const bsr_u32x4_a8 (&v)[8]) {
		const bool full = i0 + (uint32_t)(NT * 16) <= size;   // (uniform) every element of the trip exists
		const uint32_t i = i0 + 2u * (uint32_t)tid;
		take8(full, i, v, 0);
		if (i0 + 2u * (uint32_t)(4 * NT) < size) take8(full, i + 2u * (uint32_t)(4 * NT), v, 4);   // (uniform bound)
	};
	// (k_bucket_sort<2048, 1>, one workgroup per CU: requesting the next trip's loads before this one's elements are taken
	// -- two register sets -- was measured: 130 us against 117; sixteen waves of which eight sort: 128)
	for (uint32_t i0 = 0; i0 < size; i0 += NT * 16) {
		bsr_u32x4_a8 v[8];
		request(i0, v);
		consume(i0, v);
	}
	if (lane == 0 && before != 0u) atomicAdd(&s_part[0], before);   // LDS
	__syncthreads();
	// ---- layout: part-major inside the bucket's range, tiles of a part in order of L
	const uint32_t part_beg = beg + s_part[0];
	// every wave keeps the owned tiles' counts and first positions in its lanes (lane L <-> tile L): one LDS read and a
	// DPP scan instead of a serial sum of up to 16 counters per look-up
	static_assert(NA <= 64, "one lane per owned tile");
	const uint32_t cnt_lane = lane < NA ? s_cnt[lane] : 0u;
	const uint32_t first_lane = part_beg + wave_inclusive_sum_dpp(cnt_lane) - cnt_lane;
	auto tile_first = [&](int L) {   // first position of owned tile L (L wave-uniform)
		return (uint32_t)__builtin_amdgcn_readlane((int)first_lane, L);
	};
	auto tile_first_any = [&](int L) {   // the same for a lane's own L (the long-tile pass)
		uint32_t f = part_beg;
		for (int q = 0; q < L; q++) f += s_cnt[q];
		return f;
	};
	if (tid < m) tile_range[(uint32_t)((j + (tid << k_log2)) << BSR_RADIX_BITS) | (uint32_t)d] = make_uint2(first_lane, first_lane + cnt_lane);
	// ---- every wave sorts its tiles
	const bool any_long = wave_ballot(lane < m && cnt_lane > (uint32_t)AREA) != 0ull;   // (workgroup-uniform: every wave sees all counts)
	// ranks by counting, tiles of up to 64 keys ((depth bits, id) pairs are unique within a tile): no network, no further
	// LDS traffic
	auto sort_by_ranks = [&](const uint64_t* keys, int n, uint32_t start) {
		uint64_t key = ~0ull;
		if (lane < n) key = keys[swz_m<SM>(lane)];
		const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key;
		uint32_t rank = 0;
		for (int q = 0; q < n; q++) {
			const uint64_t kq = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)kh, q) << 32) |
			                    (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)kl, q);
			rank += kq < key ? 1u : 0u;
		}
		if (lane < n) point_list[start + rank] = kl;
	};
	if constexpr (TPW == 2) {
		// tiles L = wave (lanes 0..31) and wave + NW (lanes 32..63), the same schedule for both: n2 = the larger one's
		const int LA = wave, LB = wave + NW;
		int nA = LA < m ? (int)s_cnt[LA] : 0, nB = LB < m ? (int)s_cnt[LB] : 0;
		if (nA > AREA) nA = 0;   // (long: sorted further down)
		if (nB > AREA) nB = 0;
		const uint32_t startA = tile_first(LA < m ? LA : 0), startB = tile_first(LB < m ? LB : 0);
		// bucket-and-rank sort, one tile after the other with all 64 lanes (sort_mode 0); a tile it declines stays as it
		// is and goes through the network below
		if (sort_mode == 0) {
			auto by_ranks = [&](int L, int& n, uint32_t start) {
				if (n <= 64) return;
				uint64_t* const keys = s_keys + L * AREA;
				uint64_t e[AREA / 64];
#pragma unroll
				for (int q = 0; q < AREA / 64; q++) e[q] = lane + 64 * q < n ? keys[swz_m<SM>(lane + 64 * q)] : 0ull;
				round_sync<false>();
				if (rank_sort<64, AREA / 64, RNBLOG, false>(e, n, lane, keys, s_rank[wave], nullptr, start, point_list)) n = 0;
				round_sync<false>();
			};
			by_ranks(LA, nA, startA);
			by_ranks(LB, nB, startB);
		}
		if (nA <= 64 && nB <= 64) {
			if (nA > 0) sort_by_ranks(s_keys + LA * AREA, nA, startA);
			if (nB > 0) sort_by_ranks(s_keys + LB * AREA, nB, startB);
		} else {
			int n2 = 128;
			while (n2 < nA || n2 < nB) n2 <<= 1;
			const int half = lane >> 5, t = lane & 31;
			const int n = half ? nB : nA;
			const uint32_t start = half ? startB : startA;
			uint64_t* const keys = s_keys + (half ? LB : LA) * AREA;
			// pads, then runs of 16 sorted in registers, in place: a lane reads and writes the same sixteen slots
			round_sync<false>();
			for (int i = n + t; i < n2; i += 32) keys[swz_m<4>(i)] = BSR_PAD_KEY;
			round_sync<false>();
			bool plain = true;
			for (int i = t * 16; i < n2; i += 32 * 16) {
				uint64_t e[16];
				const int p0 = swz_m<4>(i);
#pragma unroll
				for (int q = 0; q < 16; q++) {
					e[q] = keys[p0 ^ swz_m<4>(q)];
					plain = plain && (i + q >= n || key_is_plain_double(e[q]));
				}
				reg_sort<4, false>(e);
#pragma unroll
				for (int q = 0; q < 16; q++) keys[p0 ^ swz_m<4>(q)] = e[q];
			}
			if (wave_ballot(!(plain && !force_int)) == 0ull)
				merge_loaded_runs<32, 4, false, true>(keys, n2, start, n, t, point_list);
			else
				merge_loaded_runs<32, 4, false, false>(keys, n2, start, n, t, point_list);
		}
	} else
	for (int L = wave; L < m; L += NW) {
		const int n = (int)s_cnt[L];
		const uint32_t start = tile_first(L);
		uint64_t* const keys = s_keys + L * AREA;
		if (n > 0 && n <= 64) {
			sort_by_ranks(keys, n, start);
		} else if (n > 64 && n <= AREA) {
			if (sort_mode == 0) {   // bucket-and-rank sort; a tile it declines goes through the network
				uint64_t e[AREA / 64];
#pragma unroll
				for (int q = 0; q < AREA / 64; q++) e[q] = lane + 64 * q < n ? keys[swz_m<SM>(lane + 64 * q)] : 0ull;
				round_sync<false>();
				const bool done = rank_sort<64, AREA / 64, RNBLOG, false>(e, n, lane, keys, s_rank[wave], nullptr, start, point_list);
				round_sync<false>();
				if (done) continue;
			}
			int n2 = 128;
			while (n2 < n) n2 <<= 1;
			// pads, then runs of 8 sorted in registers, in place: a lane reads and writes the same eight slots
			round_sync<false>();
			for (int i = n + lane; i < n2; i += 64) keys[swz_m<3>(i)] = BSR_PAD_KEY;
			round_sync<false>();
			bool plain = true;
			for (int i = lane * 8; i < n2; i += 64 * 8) {
				uint64_t e[8];
				const int p0 = swz_m<3>(i);
#pragma unroll
				for (int q = 0; q < 8; q++) {
					e[q] = keys[p0 ^ swz_m<3>(q)];
					plain = plain && (i + q >= n || key_is_plain_double(e[q]));
				}
				reg_sort<3, false>(e);
#pragma unroll
				for (int q = 0; q < 8; q++) keys[p0 ^ swz_m<3>(q)] = e[q];
			}
			if (wave_ballot(!(plain && !force_int)) == 0ull)
				merge_loaded_runs<64, 3, false, true>(keys, n2, start, n, lane, point_list);
			else
				merge_loaded_runs<64, 3, false, false>(keys, n2, start, n, lane, point_list);
		}
	}
	if (!any_long) return;
	// ---- long tiles of this part: a second pass over the bucket stages their keys in global scratch, at the segment's
	// own positions; then the whole workgroup sorts them one by one
	__syncthreads();
	if (tid < NA) s_cur[tid] = 0u;
	__syncthreads();
	for (uint32_t i0 = 0; i0 < size; i0 += NT * 4) {
		uint2 v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const uint32_t i = i0 + (uint32_t)(u * NT + tid);
			v[u] = i < size ? src[i] : make_uint2(0u, 0u);
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const uint32_t i = i0 + (uint32_t)(u * NT + tid);
			if (i < size) {
				const uint32_t hi = v[u].x >> 24;
				const uint32_t L = hi >> k_log2;
				if ((int)(hi & (uint32_t)(k - 1)) == j && s_cnt[L] > (uint32_t)AREA) {
					const uint32_t pos = atomicAdd(&s_cur[L], 1u);   // LDS
					big_keys[(size_t)tile_first_any((int)L) + pos] = ((uint64_t)v[u].y << 32) | (uint64_t)(v[u].x & 0x00ffffffu);
				}
			}
		}
	}
	__threadfence();
	__syncthreads();
	const RawKeys raw{big_keys};
	for (int L = 0; L < m; L++) {
		const int n = (int)s_cnt[L];
		if (n <= AREA) continue;   // (uniform)
		const uint32_t start = tile_first(L);
		if (n <= BSR_SORT_CHUNK)
			sort_long_tile_lds<NT>(s_keys, &s_rank[0][0], start, n, tid, raw, point_list, sort_mode);
		else
			sort_long_tile_hybrid<NT>(s_keys, big_keys + start, start, n, tid, raw, point_list);
	}
}

// k_bucket_sort<AREA, TPW> over the 256 pass-1 buckets, each split over 2^k_log2 workgroups that own NW * TPW tiles each
template <int AREA, int TPW>
static void launch_bucket_sort(int T, const int* n_ptr, int capacity, const uint32_t* digit_total1, const BinElem* elems,
                               uint2* tile_range, uint64_t* big_keys, uint32_t* point_list, int sort_mode, hipStream_t s)
{
	const int nt_max = (T + BSR_RADIX_BINS - 1) / BSR_RADIX_BINS;   // tiles of a bucket
	int k_log2 = 0;
	while ((TPW * BSR_BKT_NW << k_log2) < nt_max) k_log2++;
	hipLaunchKernelGGL((k_bucket_sort<AREA, TPW>), dim3(BSR_RADIX_BINS << k_log2), dim3(BSR_BKT_NT), 0, s, T, k_log2, n_ptr,
	                   capacity, digit_total1, elems, tile_range, big_keys, point_list, sort_mode);
}

// Size classes: (0, 1024] -> one WAVE per tile (8 KB of LDS each); the wide classes share ONE launch
// (k_sort_tiles_wide): (1024, 4096] sorted in 32 KB of LDS, longer segments hybrid in 4096-key chunks, one entry of a
// work list per workgroup.  n instances can fill at most n / 1024 (n / 4096) such tiles, which bounds the grid: a frame
// without long lists pays one near-empty launch, not 3 x T idle workgroups.
void launch_sort_tiles(const BinPlan& plan, int T, int n_bound, const int* n_ptr, int capacity, uint2* tile_range,
                       const uint32_t* big_tiles, const int* flags, const uint32_t* digit_total1, const BinElem* elems,
                       BinElem* elems_free, uint32_t* point_list, int force_int, int small_grids_flag, hipStream_t s)
{
	// force_int = the call's sort mode: bit 0 BSR_FLAG_TEST_SORT_INT, bit 1 BSR_FLAG_TEST_SORT_NETWORK (0: bucket-and-rank
	// sort first, the network for the segments it declines); small_grids_flag: BSR_FLAG_TEST_SMALL_GRIDS (test-only, no result
	// changes): every segment through the integer compare-exchange flavour, which real inputs reach only with NaN /
	// non-positive depth bits; the wide classes on grids of 2 / 1 workgroups
	switch (plan.form) {
	case BinPlan::BUCKET: {
		// second pass + sort in one launch: `elems` is still in pass-1 order; the free buffer holds the keys of long tiles.
		// 72 KB of LDS -- 16 tile areas of 512 keys (two per wave) or 8 of 1024 -- or 144 KB (8 areas of 2048: gfx950's
		// 160 KB); a bucket has ceil(T / 256) tiles, split over k = 1, 2 or 4 workgroups.
		uint64_t* const big_keys = reinterpret_cast<uint64_t*>(elems_free);
		if (plan.area == 512)
			launch_bucket_sort<512, 2>(T, n_ptr, capacity, digit_total1, elems, tile_range, big_keys, point_list, force_int, s);
		else if (plan.area == 1024)
			launch_bucket_sort<1024, 1>(T, n_ptr, capacity, digit_total1, elems, tile_range, big_keys, point_list, force_int, s);
		else
			launch_bucket_sort<2048, 1>(T, n_ptr, capacity, digit_total1, elems, tile_range, big_keys, point_list, force_int, s);
		return;
	}
	case BinPlan::CHAIN:
	case BinPlan::RADIX:
		break;   // the segments lie in tile order: one launch per size class
	}
	const int compact = plan.compact;
	// sparse frames (the views of a camera sweep: every tile a few dozen entries) get the tiny class its own kernel;
	// where tiles average 128 entries or more the few short ones stay with the small class (one launch fewer)
	const bool tiny = (long long)n_bound < 128ll * T;
	if (tiny)
		hipLaunchKernelGGL(k_sort_tiles_tiny, dim3((T + 3) / 4), dim3(256), 0, s, T, n_ptr, capacity, tile_range, elems,
		                   point_list, compact);
	hipLaunchKernelGGL(k_sort_tiles_small, dim3((T + 3) / 4), dim3(256), 0, s, T, n_ptr, capacity, tile_range, elems, point_list,
	                   force_int, tiny ? 64 : 0, compact);
	// n instances can fill at most n / 1025 tiles of the first wide class and n / 4097 of the two longer ones: the grid
	// covers both work lists (n_bound >= the real count), capped -- the workgroups stride over their lists
	// (BSR_FLAG_TEST_SMALL_GRIDS: caps of 2 / 1, so that ordinary test frames drive several tiles through one
	// workgroup's striding loop -- with the product caps that takes > 2560 / 512 long tiles in one frame)
	const bool small_grids = small_grids_flag != 0;
	const int g1 = min(min(T, n_bound / (BSR_SORT_SMALL + 1)), small_grids ? 2 : 2560),
	          gw = min(min(T, n_bound / (BSR_SORT_CHUNK + 1)), small_grids ? 1 : 512);
	// (1024, 2048] in a launch of its own where the frame can hold a fair number of such tiles (a dense frame); a frame
	// of short lists pays no second near-empty launch.  The first wide class then starts at 2049 keys: at most
	// n / 2049 such tiles, and its near-empty launch is kept small (2560 workgroups of 512 that find nothing: 10 us).
	const bool mid = g1 >= 64 || small_grids;
	int g1w = g1;
	if (mid) {
		const int gm = small_grids ? 2 : min(g1, BSR_SORT_MID_WGS);
		hipLaunchKernelGGL(k_sort_tiles_mid, dim3(gm), dim3(256), 0, s, gm, n_ptr, capacity, tile_range, big_tiles, flags, elems,
		                   point_list, force_int, compact);
		g1w = min(min(T, n_bound / (BSR_SORT_MID + 1)), small_grids ? 2 : 640);
	}
	if (g1w + gw > 0)
		hipLaunchKernelGGL(k_sort_tiles_wide, dim3(g1w + gw), dim3(BSR_SORT_NT), 0, s, T, g1w, n_ptr, capacity, tile_range,
		                   big_tiles, flags, elems, reinterpret_cast<uint64_t*>(elems_free), point_list, force_int, compact,
		                   mid ? BSR_SORT_MID : BSR_SORT_SMALL);
}

}  // namespace bsr
