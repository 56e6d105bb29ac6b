// Binning: the scans, the instance emit and the placement of every kept instance in its tile's segment -- no
// floating-point atomics, and the few integer ones never decide a result.  (The per-tile depth sort that follows:
// tile_sort.h, tile_sort.hip.)
//
// The reference emits one 64-bit (tile | depth) key per (Gaussian, tile) instance in Gaussian order
// and runs a global stable radix sort over all R instances on 32+bit key bits, six 8-bit passes at
// 1080p (rasterizer_impl.cu:70-111,304-309 of its depth-diff-gaussian-rasterization), then finds tile ranges
// (:116-138).  The resulting order is (tile, depth bit pattern, Gaussian id).  Here:
//   1. k_preprocess decided per (Gaussian, tile) whether the splat can reach the tile at all
//      (exact conservative ellipse-vs-tile test; ~1/3 of the reference's instances are dropped on the
//      synthetic scenes, no pixel changes), numbered the kept instances inside its workgroup and
//      counted them per low tile-id byte (`hist1`, an LDS histogram per workgroup); k_scans
//      prefix-sums the workgroup totals and the 256 digit rows of hist1 (one launch),
//   2. k_emit_scatter writes every kept instance as one 12-byte element (tile id, Gaussian id,
//      depth bits) straight to its position after the FIRST radix pass: digit base + the prefix of
//      the earlier workgroups + an LDS counter.  The order inside one (workgroup, digit) group is
//      whatever the LDS atomics give -- it does not matter, see 5 (tile_sort.h),
//   3. tile ids of up to 16 bits (every single-view call up to 4096 x 4096): the tile-owned second pass further down
//      (k_tile_count -> k_tile_starts -> k_tile_scatter), which also produces the tile ranges of 4.  Otherwise:
//      the remaining ceil(bits(T)/8) - 1 stable LSD radix passes on the TILE ID only (1080p: one
//      more pass; the reference does six over 45 key bits; elements move as single 12-byte
//      loads/stores): per-workgroup digit histogram -> 256 parallel row scans -> stable scatter
//      (wave ballots for the in-round rank, stamped per-wave counters across the 4 waves),
//   4. k_tile_ranges finds each tile's segment by a 16-ary search (one DPP row of 16 lanes per tile).
// Steps 5 (every segment sorted by its 64-bit key in LDS) and 6 (steps 3-5 in ONE launch, k_bucket_sort) are
// tile_sort.hip's; binning_plan, at the end of this file, decides which form a call takes.
// The earlier version counted and appended instances with global integer atomics (~20 G/s when
// lane-scattered on MI355X: 0.2 ms at C3, 1.4 ms at C5); this one is also fully deterministic.
#include "tile_sort.h"
#include "launch.h"
#include "wg_scan.h"

namespace bsr {

// The two scans between k_preprocess and the binning, in one launch:
//  workgroup 256     : per-preprocess-workgroup totals: kept instances -> workgroup bases (in place) and
//                      flags[2] = total kept; rect tiles -> flags[3] = the reference's num_rendered,
//  workgroups 0..255 : digit d's row of hist1 (the pass-1 histogram counted by k_preprocess, digit-major, one
//                      column per preprocess workgroup, XCD-grouped) -> exclusive prefixes in place + the digit
//                      total behind the rows.  Pad columns (no workgroup) are never written and count as 0.
struct Hist1ColumnValid {
	int per, n_wg;
	__device__ __forceinline__ bool operator()(int col) const { return hist1_wg_of_column(col, per) < n_wg; }
};
__global__ void __launch_bounds__(1024) k_scans(int n_wg, uint32_t* __restrict__ wg_kept,
                                                uint32_t* __restrict__ wg_area, int* __restrict__ flags,
                                                uint32_t* __restrict__ hist1, int* __restrict__ host_counts)
{
	__shared__ uint32_t s_w[32];
	if (blockIdx.x == BSR_RADIX_BINS) {
		const uint32_t kept = wg_exclusive_scan<16, 4>(n_wg, wg_kept, s_w, true);
		const uint32_t area = wg_exclusive_scan<16, 4>(n_wg, wg_area, s_w, false);
		if (threadIdx.x == 0) {
			flags[2] = (int)kept;
			flags[3] = (int)area;
			flags[1] = flags[4] = flags[5] = 0;   // counters of k_tile_ranges (the image buffer arrives uninitialised)
			flags[6] = flags[7] = 0;
			flags[BSR_POOL_FWD] = flags[BSR_POOL_BWD] = 0;   // pool counters of the two tile walks (common.h: pooled_tile)
			if (host_counts != nullptr) {
				// the forward's one read-back (reference rasterizer_impl.cu:282), without a copy: the four counters go
				// straight into the calling thread's pinned, device-mapped landing buffer; the host waits for the event
				// recorded behind this kernel (a 16-byte hipMemcpyAsync was a 4 us operation of its own on the stream)
				host_counts[0] = flags[0];
				host_counts[1] = 0;
				host_counts[2] = (int)kept;
				host_counts[3] = (int)area;
				__threadfence_system();
			}
		}
		return;
	}
	const int per = (n_wg + 7) >> 3, n_col = 8 * per;
	const uint32_t total = wg_exclusive_scan<16, 4>(n_col, hist1 + (size_t)blockIdx.x * n_col, s_w, true,
	                                                Hist1ColumnValid{per, n_wg});
	if (threadIdx.x == 0) hist1[(size_t)BSR_RADIX_BINS * n_col + blockIdx.x] = total;   // digit totals behind the rows
}

// The binning kernels take the number of kept instances from DEVICE memory (flags[2], written by
// k_scans) and derive their work partition from it themselves, so the host can enqueue the whole
// binning stage before it has read that number back (bsr_forward overlaps its one blocking read with
// these kernels).  `capacity` is the number of instances the scratch buffers were sized for; if more
// were kept, every kernel returns at once and the host re-runs the stage with the right size.
struct RadixPartition { int n, chunk, n_blocks; };
__device__ __forceinline__ RadixPartition radix_partition(const int* __restrict__ n_ptr, int capacity,
                                                          int hist_blocks_max)
{
	RadixPartition p;
	p.n = *n_ptr;
	if (p.n > capacity || p.n < 0) p.n = -1;   // overflow: do nothing
	// chunk: multiple of 256, at least 1024 elements, at most hist_blocks_max workgroups
	int chunk = ((max(p.n, 0) + hist_blocks_max - 1) / hist_blocks_max + 255) / 256 * 256;
	p.chunk = chunk < 1024 ? 1024 : chunk;
	p.n_blocks = (max(p.n, 0) + p.chunk - 1) / p.chunk;
	return p;
}

// One workgroup per digit d: exclusive scan of row d of the digit-major histogram (in place) and the
// row total.  256 short, independent scans instead of one long latency-bound one.
__global__ void __launch_bounds__(256) k_radix_rowscan(const int* __restrict__ n_ptr, int capacity, int hist_blocks_max,
                                                       uint32_t* __restrict__ hist,
                                                       uint32_t* __restrict__ digit_total)
{
	__shared__ uint32_t s_wave[8];
	const RadixPartition part = radix_partition(n_ptr, capacity, hist_blocks_max);
	if (part.n <= 0) return;
	const uint32_t total = wg_exclusive_scan<4, 1>(part.n_blocks, hist + (size_t)blockIdx.x * part.n_blocks, s_wave, true);
	if (threadIdx.x == 0) digit_total[blockIdx.x] = total;
}

// ---- first radix pass, fused with the instance emit ----
// The per-workgroup histogram over the low 8 bits of the tile id was counted by k_preprocess (hist1,
// digit-major, one column per preprocess workgroup).  k_scans turns every digit's row into
// exclusive prefixes + the digit total; k_emit_scatter then writes each kept instance straight to its
// place in the pass-1 order: digit base + its workgroup's prefix + a running LDS counter.  The order
// inside a (workgroup, digit) bucket is arbitrary -- harmless, the per-tile sort orders by the unique
// (depth, id) key -- so no Gaussian-major staging array, no separate histogram pass.
__global__ void __launch_bounds__(256) k_emit_scatter(int P, int gx, const int* __restrict__ n_ptr, int capacity,
                                                      const ushort4* __restrict__ rect,
                                                      const uint64_t* __restrict__ kept_mask,
                                                      const float* __restrict__ depth,
                                                      const uint32_t* __restrict__ hist1,
                                                      uint32_t* __restrict__ digit_base, BinElem* __restrict__ elems,
                                                      uint32_t* __restrict__ zero_me, int n_zero, int compact)
{
	__shared__ uint32_t s_off[BSR_RADIX_BINS];   // next output position per digit for this workgroup
	__shared__ uint32_t s_scan[4];
	{
		const int n = *n_ptr;
		if (n <= 0 || n > capacity) return;
	}
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int n_wg = (int)gridDim.x, per = (n_wg + 7) >> 3, n_col = 8 * per;
	const int idx = blockIdx.x * 256 + tid;
	// counters of the tile-owned second pass (tile_count[T], tile_cursor[T]): zeroed here, one launch ahead of their use
	for (int i = idx; i < n_zero; i += n_wg * 256) zero_me[i] = 0u;
	// Everything this thread needs from global memory is requested up front: the kernel is a chain of dependent
	// round trips otherwise (totals -> barrier -> column -> barrier -> rect -> mask / depth), and loads do not move
	// across barriers on their own.  Rows of culled Gaussians hold an empty rect; their mask / depth are never
	// written, whatever is read there is not used.
	const bool in_range = idx < P;
	const int ld = in_range ? idx : 0;
	const uint32_t v = hist1[(size_t)BSR_RADIX_BINS * n_col + tid];
	const uint32_t col = hist1[(size_t)tid * n_col + hist1_column((int)blockIdx.x, per)];
	const ushort4 r = rect[ld];
	const uint64_t mask = kept_mask[ld];
	const uint32_t depth_bits = __float_as_uint(depth[ld]);
	{   // digit base = exclusive scan of the 256 digit totals (thread d <-> digit d) + this workgroup's prefix
		// (wg_scan.h: wg_exclusive_sum, kept in its own text: the call compiles to another instruction stream here)
		const uint32_t incl = wave_inclusive_sum_dpp(v);
		if (lane == 63) s_scan[wave] = incl;
		__syncthreads();
		const uint32_t base = (wave > 0 ? s_scan[0] : 0u) + (wave > 1 ? s_scan[1] : 0u) + (wave > 2 ? s_scan[2] : 0u) + incl - v;
		s_off[tid] = base + col;
		// the 256 digit bases, once, behind the digit totals: k_bucket_sort takes its bucket's range from there instead
		// of every one of its workgroups scanning the totals again (a load, a scan and two barriers at its start).
		// (digit_base = hist1 + 256 n_col + 256: words no workgroup of this kernel reads)
		if (blockIdx.x == 0) digit_base[tid] = base;
	}
	__syncthreads();
	if (!in_range) return;
	if (r.z <= r.x || r.w <= r.y) return;
	const uint32_t area = (uint32_t)(r.z - r.x) * (uint32_t)(r.w - r.y);
	if (kept_count(area, mask) == 0) return;
	uint32_t k = 0;
	for (int y = r.y; y < r.w; y++)
		for (int x = r.x; x < r.z; x++, k++) {
			if (!tile_kept(area, mask, k)) continue;
			const uint32_t tile = (uint32_t)(y * gx + x);
			const uint32_t pos = atomicAdd(&s_off[tile & (BSR_RADIX_BINS - 1)], 1u);   // LDS
			store_elem_m(elems, pos, BinElem{tile, (uint32_t)idx, depth_bits}, compact);   // one 8- or 12-B store
		}
}

// ---- stable LSD radix pass on bits [shift, shift+8) of the tile id ----
// Workgroup b owns elements [b*chunk, (b+1)*chunk).  hist is digit-major: hist[d * n_blocks + b].
__global__ void __launch_bounds__(256) k_radix_hist(const int* __restrict__ n_ptr, int capacity, int hist_blocks_max,
                                                    int shift, const BinElem* __restrict__ elems,
                                                    uint32_t* __restrict__ hist)
{
	__shared__ uint32_t s_hist[BSR_RADIX_BINS];
	const RadixPartition part = radix_partition(n_ptr, capacity, hist_blocks_max);
	if ((int)blockIdx.x >= part.n_blocks) return;   // also the overflow / empty case (n_blocks = 0)
	const int n = part.n, chunk = part.chunk, n_blocks = part.n_blocks;
	const int tid = threadIdx.x;
	s_hist[tid] = 0;
	__syncthreads();
	const int beg = blockIdx.x * chunk, end = min(n, beg + chunk);
	for (int i = beg + tid; i < end; i += 1024) {   // four loads in flight per trip (the kernel is load latency)
		uint32_t t[4];
#pragma unroll
		for (int k = 0; k < 4; k++) t[k] = (i + 256 * k < end) ? elems[i + 256 * k].x : 0u;
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (i + 256 * k < end) atomicAdd(&s_hist[(t[k] >> shift) & (BSR_RADIX_BINS - 1)], 1u);
	}
	__syncthreads();
	hist[(size_t)tid * n_blocks + blockIdx.x] = s_hist[tid];
}

__global__ void __launch_bounds__(256) k_radix_scatter(const int* __restrict__ n_ptr, int capacity,
                                                       int hist_blocks_max, int shift,
                                                       const BinElem* __restrict__ elems_in,
                                                       BinElem* __restrict__ elems_out,
                                                       const uint32_t* __restrict__ hist,
                                                       const uint32_t* __restrict__ digit_total)
{
	__shared__ uint32_t s_off[BSR_RADIX_BINS];        // next output position per digit for this workgroup
	__shared__ uint32_t s_wcnt[4][BSR_RADIX_BINS];    // (round << 8 | count) per wave and digit, stamped
	__shared__ uint32_t s_scan[4];
	const RadixPartition part = radix_partition(n_ptr, capacity, hist_blocks_max);
	if ((int)blockIdx.x >= part.n_blocks) return;
	const int n = part.n, chunk = part.chunk, n_blocks = part.n_blocks;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int beg = blockIdx.x * chunk, end = min(n, beg + chunk);
	// requested before the first barrier (loads do not move across barriers on their own): this block's row of
	// prefixes and the first round's element; inside the loop the next round's element is always in flight
	const uint32_t row_prefix = hist[(size_t)tid * n_blocks + blockIdx.x];
	BinElem e_next = BinElem{0u, 0u, 0u};
	if (beg + tid < end) e_next = load_elem(elems_in + beg + tid);
	{   // digit base = exclusive scan of the 256 digit totals (thread d <-> digit d) + this block's row prefix
		s_off[tid] = wg_exclusive_sum<4>(digit_total[tid], s_scan) + row_prefix;
	}
#pragma unroll
	for (int w = 0; w < 4; w++) s_wcnt[w][tid] = 0;
	__syncthreads();
	const unsigned long long lt = (1ull << lane) - 1ull;
	uint32_t round = 1;
	for (int base = beg; base < end; base += 256, round++) {
		const int i = base + tid;
		const bool valid = i < end;
		const BinElem e = e_next;
		if (i + 256 < end) e_next = load_elem(elems_in + i + 256);
		const uint32_t d = (e.x >> shift) & (BSR_RADIX_BINS - 1);
		// lanes of this wave with the same digit (invalid lanes match nobody)
		unsigned long long peers = __ballot(valid);
#pragma unroll
		for (int b = 0; b < BSR_RADIX_BITS; b++) {
			const bool bit = (d >> b) & 1u;
			const unsigned long long m = __ballot(bit);
			peers &= bit ? m : ~m;
		}
		const uint32_t rank_w = (uint32_t)__popcll(peers & lt);
		const uint32_t cnt_w = (uint32_t)__popcll(peers);
		if (valid && rank_w == 0) s_wcnt[wave][d] = (round << 8) | cnt_w;
		__syncthreads();
		uint32_t lower = 0;
		if (valid) {
#pragma unroll
			for (int w = 0; w < 4; w++) {
				const uint32_t c = s_wcnt[w][d];
				if (w < wave && (c >> 8) == round) lower += c & 0xffu;
			}
			const uint32_t pos = s_off[d] + lower + rank_w;
			store_elem(elems_out + pos, e);
		}
		__syncthreads();
		if (valid && rank_w == 0) atomicAdd(&s_off[d], cnt_w);   // LDS; order irrelevant, positions are taken
	}
}

// ---- second pass for tile ids of up to 16 bits: per-tile counts -> tile starts -> scatter to the tile's segment ----
// The order INSIDE a tile is free (the per-tile sort orders by the unique (depth, id) key), so the last pass needs
// neither a stable scatter nor a histogram per workgroup: after pass 1 the instances of tile t all sit in bucket
// t & 255, and
//   k_tile_count   : workgroups (bucket d1, slice s) count their slice by the high byte in LDS and add the non-zero
//                    bins to tile_count[t] (a few thousand global integer atomics in all),
//   k_tile_starts  : ONE workgroup turns the counts into tile_start[0 .. T] (exclusive scan in tile order) and files
//                    the tiles of the wide sort classes -- the 16-ary search of k_tile_ranges and its dependent
//                    loads through a 36 .. 180 MB array are gone,
//   k_tile_scatter : the same workgroups recount their slice, reserve a range in each tile they touch (one returning
//                    atomic per non-zero bin) and move their elements there (LDS cursors; no ballots, no barriers
//                    inside the loop).
// Against histogram + row scan + stable scatter + search (A/B on one box): binning C3 0.071 -> 0.064 ms, C5 0.333 ->
// 0.309, dense 0.193 -> 0.180, C2 0.022 -> 0.018.
struct BucketSlice { int beg, end; };
// [beg, end) of slice `s` (of n_slices) of pass-1 bucket d1; thread d holds digit d's total (256 threads)
__device__ __forceinline__ BucketSlice bucket_slice(uint32_t my_total, int d1, int s, int n_slices, uint32_t* s_scan,
                                                    uint32_t* s_base)
{
	const int tid = threadIdx.x;
	const uint32_t base = wg_exclusive_sum<4>(my_total, s_scan);
	if (tid == d1) {
		s_base[0] = base;
		s_base[1] = my_total;
	}
	__syncthreads();
	const uint32_t b0 = s_base[0], size = s_base[1];
	const uint32_t len = ((size + (uint32_t)n_slices - 1) / (uint32_t)n_slices + 255u) & ~255u;   // multiple of 256
	BucketSlice r;
	r.beg = (int)(b0 + min(size, (uint32_t)s * len));
	r.end = (int)(b0 + min(size, (uint32_t)(s + 1) * len));
	return r;
}

// LDS histogram of the high byte over elems[beg, end): four loads in flight per trip
__device__ __forceinline__ void slice_histogram(const BinElem* __restrict__ elems, BucketSlice sl, uint32_t* s_hist, int compact)
{
	const int tid = threadIdx.x;
	for (int i = sl.beg + tid; i < sl.end; i += 1024) {
		uint32_t t[4];
#pragma unroll
		for (int k = 0; k < 4; k++) t[k] = (i + 256 * k < sl.end) ? elem_tile_m(elems, (size_t)(i + 256 * k), compact) : 0u;
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (i + 256 * k < sl.end) atomicAdd(&s_hist[(t[k] >> BSR_RADIX_BITS) & (BSR_RADIX_BINS - 1)], 1u);
	}
}

__global__ void __launch_bounds__(256) k_tile_count(int T, int n_slices, const int* __restrict__ n_ptr, int capacity,
                                                    const uint32_t* __restrict__ digit_total1,
                                                    const BinElem* __restrict__ elems, uint32_t* __restrict__ tile_count,
                                                    int compact)
{
	__shared__ uint32_t s_hist[BSR_RADIX_BINS];
	__shared__ uint32_t s_scan[4];
	__shared__ uint32_t s_base[2];
	{
		const int n = *n_ptr;
		if (n <= 0 || n > capacity) return;
	}
	const int tid = threadIdx.x;
	const int d1 = (int)blockIdx.x / n_slices, s = (int)blockIdx.x % n_slices;
	s_hist[tid] = 0;
	const BucketSlice sl = bucket_slice(digit_total1[tid], d1, s, n_slices, s_scan, s_base);   // (barriers inside)
	slice_histogram(elems, sl, s_hist, compact);
	__syncthreads();
	const uint32_t c = s_hist[tid];
	const uint32_t t = ((uint32_t)tid << BSR_RADIX_BITS) | (uint32_t)d1;
	if (c != 0u && t < (uint32_t)T) atomicAdd(&tile_count[t], c);
}

// ONE workgroup of 1024: tile_count -> tile_start (exclusive scan in tile order, tile_start[T] = total) and the work
// lists of the wide sort classes (as k_tile_ranges builds them).  (Folding this into k_tile_count's last-finishing
// workgroup was measured: the per-workgroup ordering it needs -- returning atomics + one contended counter -- cost 4x
// the launch it saves.)  The tiles are taken in chunks of 1024 consecutive ones, thread i <-> tile 1024 j + i: every
// access is coalesced (a thread owning `per` CONSECUTIVE tiles made each wave load touch 64 cache lines: 105 us on
// this one CU at 65 536 tiles -- 8 stacked 1080p views, one 8K view).  All counts are requested up front and stay in
// registers; a wave scans its 64 tiles of every chunk, then the 16 x (chunks) wave totals are scanned once.
template <int NC>   // chunks held in registers: 8 (up to 8192 tiles: one 1080p view) or 64 (16-bit tile ids)
__global__ void __launch_bounds__(1024) k_tile_starts(int T, const int* __restrict__ n_ptr, int capacity,
                                                      const uint32_t* __restrict__ tile_count,
                                                      uint2* __restrict__ tile_range,
                                                      uint32_t* __restrict__ big_tiles, int* __restrict__ flags)
{
	__shared__ uint32_t s_tot[1024];         // [chunk][wave] totals (NC x 16 used), then their exclusive prefix
	__shared__ uint32_t s_w[16];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int chunks = (T + 1023) >> 10;     // <= NC
	uint32_t c[NC];
#pragma unroll
	for (int j = 0; j < NC; j++) c[j] = (j < chunks && (j << 10) + tid < T) ? tile_count[(j << 10) + tid] : 0u;
	{
		const int n = *n_ptr;
		if (n > capacity) return;   // overflow: the stage is re-run
		if (n <= 0) {               // nothing kept: every tile is empty (the counts were not even zeroed)
			for (int t = tid; t < T; t += 1024) tile_range[t] = make_uint2(0u, 0u);
			return;
		}
	}
	// inclusive scan of every chunk's 64 tiles of this wave (c[j] becomes the inclusive sum, the count is re-derived)
	bool any_big = false;
	s_tot[tid] = 0u;
	__syncthreads();
#pragma unroll
	for (int j = 0; j < NC; j++) {
		if (j < chunks) {   // (uniform)
			any_big = any_big || c[j] > (uint32_t)BSR_SORT_SMALL_N;
			const uint32_t incl = wave_inclusive_sum_dpp(c[j]);
			if (lane == 63) s_tot[j * 16 + wave] = incl;
			c[j] = incl - c[j];   // exclusive within the wave
		}
	}
	__syncthreads();
	// exclusive scan of the 1024 (chunk, wave) totals: thread t owns total t
	{
		const uint32_t mine = s_tot[tid];
		const uint32_t incl = wave_inclusive_sum_dpp(mine);
		if (lane == 63) s_w[wave] = incl;
		__syncthreads();
		uint32_t run = incl - mine;
		for (int w = 0; w < wave; w++) run += s_w[w];
		s_tot[tid] = run;
	}
	__syncthreads();
#pragma unroll
	for (int j = 0; j < NC; j++)
		if (j < chunks && (j << 10) + tid < T) {
			const uint32_t first = s_tot[j * 16 + wave] + c[j];
			tile_range[(j << 10) + tid] = make_uint2(first, first + tile_count[(j << 10) + tid]);   // (the count: an L2 hit)
		}
	if (__syncthreads_or(any_big)) {   // the filing re-reads the counts
		// list positions from LDS counters (this is the only workgroup): a returning GLOBAL atomic per wave, chunk and
		// class was 8 us of this kernel's 12 on the dense leg, where most tiles are long
		__shared__ int s_cls[3];
		if (tid < 3) s_cls[tid] = 0;
		__syncthreads();
		for (int j = 0; j < chunks; j++) {
			const int t = (j << 10) + tid;
			const uint32_t cc = t < T ? tile_count[t] : 0u;
			const int cls = cc > 8192u ? 2 : (cc > 4096u ? 1 : (cc > (uint32_t)BSR_SORT_SMALL_N ? 0 : -1));
#pragma unroll
			for (int c3 = 0; c3 < 3; c3++) {
				const uint64_t b = wave_ballot(cls == c3);
				if (b == 0ull) continue;
				int base = 0;
				if (lane == 0) base = atomicAdd(&s_cls[c3], __popcll(b));   // LDS
				base = __shfl(base, 0);
				if (cls == c3) big_tiles[(size_t)c3 * T + base + __popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)t;
			}
		}
		__syncthreads();
		if (tid < 3) flags[tid == 0 ? 1 : 3 + tid] = s_cls[tid];   // (zero until now: k_scans / the re-run's memset)
	}
}

#define BSR_SLICE_REGS 16   // elements per thread held in registers by k_tile_scatter: slices of up to 4096 are read once
__global__ void __launch_bounds__(256) k_tile_scatter(int T, int n_slices, const int* __restrict__ n_ptr, int capacity,
                                                      const uint32_t* __restrict__ digit_total1,
                                                      const BinElem* __restrict__ elems_in,
                                                      BinElem* __restrict__ elems_out,
                                                      const uint2* __restrict__ tile_range,
                                                      uint32_t* __restrict__ tile_cursor, int compact)
{
	__shared__ uint32_t s_hist[BSR_RADIX_BINS];
	__shared__ uint32_t s_off[BSR_RADIX_BINS];
	__shared__ uint32_t s_scan[4];
	__shared__ uint32_t s_base[2];
	{
		const int n = *n_ptr;
		if (n <= 0 || n > capacity) return;
	}
	const int tid = threadIdx.x;
	const int d1 = (int)blockIdx.x / n_slices, s = (int)blockIdx.x % n_slices;
	s_hist[tid] = 0;
	const BucketSlice sl = bucket_slice(digit_total1[tid], d1, s, n_slices, s_scan, s_base);
	if (sl.beg >= sl.end) return;   // (uniform)
	const bool in_regs = sl.end - sl.beg <= 256 * BSR_SLICE_REGS;   // (uniform) the usual case
	BinElem e[BSR_SLICE_REGS];
	if (in_regs) {
#pragma unroll
		for (int k = 0; k < BSR_SLICE_REGS; k++) {
			const int i = sl.beg + tid + 256 * k;
			e[k] = i < sl.end ? load_elem_m(elems_in, (size_t)i, compact) : BinElem{0u, 0u, 0u};
		}
#pragma unroll
		for (int k = 0; k < BSR_SLICE_REGS; k++)
			if (sl.beg + tid + 256 * k < sl.end) atomicAdd(&s_hist[(e[k].x >> BSR_RADIX_BITS) & (BSR_RADIX_BINS - 1)], 1u);
	} else {
		slice_histogram(elems_in, sl, s_hist, compact);
	}
	__syncthreads();
	{
		const uint32_t c = s_hist[tid];
		const uint32_t t = ((uint32_t)tid << BSR_RADIX_BITS) | (uint32_t)d1;
		uint32_t off = 0;
		if (c != 0u && t < (uint32_t)T) off = tile_range[t].x + atomicAdd(&tile_cursor[t], c);
		s_off[tid] = off;
	}
	__syncthreads();
	if (in_regs) {
#pragma unroll
		for (int k = 0; k < BSR_SLICE_REGS; k++)
			if (sl.beg + tid + 256 * k < sl.end) {
				const uint32_t pos = atomicAdd(&s_off[(e[k].x >> BSR_RADIX_BITS) & (BSR_RADIX_BINS - 1)], 1u);   // LDS
				store_elem_m(elems_out, pos, e[k], compact);
			}
		return;
	}
	for (int i = sl.beg + tid; i < sl.end; i += 1024) {
		BinElem f[4];
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (i + 256 * k < sl.end) f[k] = load_elem_m(elems_in, (size_t)(i + 256 * k), compact);
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (i + 256 * k < sl.end) {
				const uint32_t pos = atomicAdd(&s_off[(f[k].x >> BSR_RADIX_BITS) & (BSR_RADIX_BINS - 1)], 1u);   // LDS
				store_elem_m(elems_out, pos, f[k], compact);
			}
	}
}

// ---- tile ranges: tile_start[t] = first sorted position whose tile id is >= t ----
// Tiles holding more than BSR_SORT_SMALL instances are also appended (one atomic per wave, order
// irrelevant) to the work list of their size class (see below); flags[1], [4], [5] count them.
// First index in [0, n) whose tile id is >= t, found by the 16 lanes of a DPP row together: every round the lanes
// probe 16 evenly spaced positions of the remaining range (one dependent L2 load per round, 17-fold narrowing:
// 6 rounds for 3 M elements instead of the 22 of a binary search -- the kernel is pure load latency).
__device__ __forceinline__ int first_not_below_row16(const BinElem* __restrict__ elems_sorted, int n, uint32_t t,
                                                     int lane)
{
	const int j = lane & 15, sh = lane & 48;
	int lo = 0, hi = n;
	while (hi > lo) {   // uniform over the row; rows of one wave may need different round counts
		const int width = hi - lo;
		if (width <= 16) {
			const bool below = j < width && elems_sorted[lo + j].x < t;
			lo += __popc((uint32_t)(wave_ballot(below) >> sh) & 0xffffu);
			break;
		}
		const int p = lo + (int)(((uint64_t)width * (uint32_t)(j + 1)) / 17u);   // lo < p < hi, ascending in j
		const bool below = elems_sorted[p].x < t;
		const int c = __popc((uint32_t)(wave_ballot(below) >> sh) & 0xffffu);   // probes 0 .. c-1 are below t
		const int new_lo = c > 0 ? lo + (int)(((uint64_t)width * (uint32_t)c) / 17u) + 1 : lo;
		const int new_hi = c < 16 ? lo + (int)(((uint64_t)width * (uint32_t)(c + 1)) / 17u) : hi;
		lo = new_lo;
		hi = new_hi;
	}
	return lo;
}

// One wave per three tiles: row k (16 lanes) finds the start of tile 3w + k, k = 0..3; rows 0..2 own their tile
// (range written, size class decided with the next row's start as the end), row 3 only delivers the end of tile
// 3w + 2.
__global__ void __launch_bounds__(256) k_tile_ranges(int T, const int* __restrict__ n_ptr, int capacity,
                                                     const BinElem* __restrict__ elems_sorted,
                                                     uint2* __restrict__ tile_range,
                                                     uint32_t* __restrict__ big_tiles, int* __restrict__ flags)
{
	int n = *n_ptr;
	if (n > capacity) return;   // overflow: the stage is re-run
	if (n < 0) n = 0;
	const int lane = threadIdx.x & 63, row = lane >> 4;
	const int wave = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
	const int t = wave * 3 + row;
	bool big = false;
	int cnt_t = 0;
	{
		const int lo = (t <= T) ? first_not_below_row16(elems_sorted, n, (uint32_t)t, lane) : n;
		const int hi = __shfl_down(lo, 16, 64);   // the next row's start
		const bool owner = row < 3 && (lane & 15) == 0;
		if (owner && t < T) {
			tile_range[t] = make_uint2((uint32_t)lo, (uint32_t)hi);
			cnt_t = hi - lo;
			big = cnt_t > BSR_SORT_SMALL;
		}
	}
	// one work list per size class of the wide sort kernels (their grids are bounded per class):
	// class 0: (1024, 4096] -> big_tiles[0..T), count flags[1]; class 1: (4096, 8192] -> [T..2T), flags[4];
	// class 2: > 8192 -> [2T..3T), flags[5]
	int cls = -1;
	if (big) cls = cnt_t > 8192 ? 2 : (cnt_t > 4096 ? 1 : 0);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const uint64_t b = __ballot(cls == k);
		if (b == 0) continue;
		int base = 0;
		if (lane == 0) base = atomicAdd(&flags[k == 0 ? 1 : 3 + k], __popcll(b));
		base = __shfl(base, 0);
		if (cls == k) big_tiles[(size_t)k * T + base + __popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)t;
	}
}

// once per forward call, right after k_preprocess (independent of the instance count: runs before the read-back)
void launch_scans(int n_wg, uint32_t* wg_kept, uint32_t* wg_area, int* flags, uint32_t* hist1, int* host_counts,
                  hipStream_t s)
{
	hipLaunchKernelGGL(k_scans, dim3(BSR_RADIX_BINS + 1), dim3(1024), 0, s, n_wg, wg_kept, wg_area, flags, hist1,
	                   host_counts);
}

// Which second pass a forward call runs (launch.h: BinPlan) -- decided on the host from sizes alone, every plan is correct
// for every input:
//   RADIX          tile ids beyond 16 bits (stacked views, > 4096 x 4096): the remaining LSD radix passes + k_tile_ranges,
//   CHAIN          tile-owned chain: k_tile_count -> k_tile_starts -> k_tile_scatter, then the per-tile sort launches,
//   BUCKET 1024x1  k_bucket_sort<1024, 1> (one launch for the second pass AND the sort): up to 8192 tiles, Gaussian ids
//      below 2^24, and lists that are short on average -- a workgroup streams its whole bucket, up to four workgroups per
//      bucket: that pays while an average tile holds well under the 1024 keys of a tile area (C3: 366 kept instances per
//      tile; the dense leg: 1600, C5: 1850),
//   BUCKET 512x2   k_bucket_sort<512, 2>: the same with 512-key areas, two tiles per wave (half the workgroups per bucket),
//      where the average tile holds at most BSR_BKT_SMALL_PER_TILE,
//   BUCKET 2048x1  k_bucket_sort<2048, 1>: 2048-key areas (128 KB of keys: one workgroup per CU, four workgroups per
//      bucket of a 1080p frame) for dense frames, up to BSR_BKT_BIG_PER_TILE per tile on average: against the chain it
//      saves the count, the global scan and the scatter (the elements written and read once more) for three more reads
//      of the bucket from the L2.
// kept_hint = the number of kept instances the caller expects (this frame's count when the host has read it, the
// previous frame's while it guesses), 0 = unknown: 70 % of the scratch capacity then (the exact tile cull keeps ~2/3
// of the reference's instances on the synthetic scenes).
// The debug builds libbsr_chain_only.so / libbsr_bucket_always.so / libbsr_bucket_big.so (csrc/Makefile) pin CHAIN /
// BUCKET 1024x1 or 512x2 / BUCKET 2048x1 for the tests by redefining the thresholds below.
#ifndef BSR_BUCKET_MAX_PER_TILE
#define BSR_BUCKET_MAX_PER_TILE 850   // (A/B on one box, both forms forced: 512 x 512 with ~750 per tile +2.8 % of the step with
                                      // the bucket form; the dense leg, 1200 per tile -- most tiles past their area -- -21 %)
#endif
#ifndef BSR_BKT_SMALL_PER_TILE
#define BSR_BKT_SMALL_PER_TILE 400
#endif
#ifndef BSR_BKT_BIG_PER_TILE
#define BSR_BKT_BIG_PER_TILE 1400   // up to here: 2048-key areas, one workgroup of 144 KB per CU.  (A/B, all forms forced:
                                    // dense leg, 1213 per tile: second pass + sorts 216 us against the chain's 240; 925 per tile:
                                    // even; C5, 1830 per tile with tiles past 2048: even, and 20 % slower at 2000 per tile)
#endif
BinPlan binning_plan(int P, int T, int capacity, long long kept_hint)
{
	int bits = 0;
	while ((1 << bits) < T) bits++;
	const bool tile_owned = bits <= 2 * BSR_RADIX_BITS && 2 * (size_t)T <= (size_t)BSR_RADIX_BINS * BSR_HIST_BLOCKS_MAX;
	// 8-byte elements where a tile-owned pass runs and Gaussian ids fit 24 bits (common.h: load_elem_m)
	const int compact = (tile_owned && P <= (1 << 24)) ? 1 : 0;
	if (!tile_owned) return BinPlan{BinPlan::RADIX, 0, compact};
	const long long kept = kept_hint > 0 ? kept_hint : (long long)capacity * 7 / 10;
	if (P <= (1 << 24) && T <= 8192 && kept <= (long long)BSR_BUCKET_MAX_PER_TILE * T)
		return kept <= (long long)BSR_BKT_SMALL_PER_TILE * T ? BinPlan{BinPlan::BUCKET, 512, compact}
		                                                     : BinPlan{BinPlan::BUCKET, 1024, compact};
	if (P <= (1 << 24) && T <= 8192 && BSR_BUCKET_MAX_PER_TILE > 0 && kept <= (long long)BSR_BKT_BIG_PER_TILE * T)
		return BinPlan{BinPlan::BUCKET, 2048, compact};
	return BinPlan{BinPlan::CHAIN, 0, compact};
}

// Bins the kept instances (their number is read from *n_ptr on the device): emit -> second pass on the tile id -> tile
// ranges (BUCKET: the second pass is part of launch_sort_tiles).  elems_a / elems_b ping-pong; *elems_sorted is the
// buffer the sort stage reads.  Grids are sized for `capacity` instances; workgroups beyond the real count exit.
void launch_binning(const BinPlan& plan, int P, int T, int gx, const int* n_ptr, int capacity, const GeomState& geom,
                    BinElem* elems_a, BinElem* elems_b, uint32_t* hist, int hist_blocks_max, uint2* tile_range,
                    uint32_t* big_tiles, int* flags, BinElem** elems_sorted, BinElem** elems_free, hipStream_t s)
{
	// pass 1 (tile id bits 0..7) fused with the emit; geom.hist1 was row-scanned by launch_scans, its 256 digit totals lie
	// behind the rows and the 256 digit bases behind those
	const int compact = plan.compact;
	const int n_wg = (P + 255) / 256, n_col = 8 * ((n_wg + 7) >> 3);
	uint32_t* const digit_total1 = geom.hist1 + (size_t)BSR_RADIX_BINS * n_col;
	uint32_t* tile_count = hist;          // [T]   (the histogram area of the generic passes, unused on this path)
	uint32_t* tile_cursor = hist + T;     // [T]
	hipLaunchKernelGGL(k_emit_scatter, dim3((P + 255) / 256), dim3(256), 0, s, P, gx, n_ptr, capacity, geom.rect,
	                   geom.kept_mask, geom.depth, geom.hist1, digit_total1 + BSR_RADIX_BINS, elems_a, tile_count,
	                   plan.form == BinPlan::CHAIN ? 2 * T : 0, compact);
	switch (plan.form) {
	case BinPlan::BUCKET:   // the bucket-owned second pass is fused with the sort (launch_sort_tiles)
		*elems_sorted = elems_a;
		*elems_free = elems_b;
		return;
	case BinPlan::CHAIN: {
		// tile ids of up to 16 bits (every single-view call up to 4096 x 4096): count -> starts -> scatter
		// slices of ~3000 elements at full capacity: k_tile_scatter holds up to 4096 in registers (one read of the
		// slice), and the global atomics stay at a few per hundred elements
		int n_slices = capacity / (BSR_RADIX_BINS * 3072) + 1;
		n_slices = n_slices > 256 ? 256 : n_slices;
		hipLaunchKernelGGL(k_tile_count, dim3(BSR_RADIX_BINS * n_slices), dim3(256), 0, s, T, n_slices, n_ptr, capacity,
		                   digit_total1, elems_a, tile_count, compact);
		if (T <= 8192)
			hipLaunchKernelGGL(k_tile_starts<8>, dim3(1), dim3(1024), 0, s, T, n_ptr, capacity, tile_count, tile_range,
			                   big_tiles, flags);
		else
			hipLaunchKernelGGL(k_tile_starts<64>, dim3(1), dim3(1024), 0, s, T, n_ptr, capacity, tile_count, tile_range,
			                   big_tiles, flags);
		hipLaunchKernelGGL(k_tile_scatter, dim3(BSR_RADIX_BINS * n_slices), dim3(256), 0, s, T, n_slices, n_ptr, capacity,
		                   digit_total1, elems_a, elems_b, tile_range, tile_cursor, compact);
		*elems_sorted = elems_b;
		*elems_free = elems_a;
		return;
	}
	case BinPlan::RADIX:
		break;
	}
	int bits = 0;
	while ((1 << bits) < T) bits++;
	int max_blocks = (capacity + 1023) / 1024;   // chunk >= 1024
	if (max_blocks > hist_blocks_max) max_blocks = hist_blocks_max;
	if (max_blocks < 1) max_blocks = 1;
	uint32_t* digit_total = hist + (size_t)BSR_RADIX_BINS * hist_blocks_max;
	BinElem* ei = elems_a; BinElem* eo = elems_b;
	for (int shift = BSR_RADIX_BITS; shift < bits; shift += BSR_RADIX_BITS) {
		hipLaunchKernelGGL(k_radix_hist, dim3(max_blocks), dim3(256), 0, s, n_ptr, capacity, hist_blocks_max, shift, ei,
		                   hist);
		hipLaunchKernelGGL(k_radix_rowscan, dim3(BSR_RADIX_BINS), dim3(256), 0, s, n_ptr, capacity, hist_blocks_max, hist,
		                   digit_total);
		hipLaunchKernelGGL(k_radix_scatter, dim3(max_blocks), dim3(256), 0, s, n_ptr, capacity, hist_blocks_max, shift, ei,
		                   eo, hist, digit_total);
		BinElem* tt = ei; ei = eo; eo = tt;
	}
	// one wave per three tiles
	hipLaunchKernelGGL(k_tile_ranges, dim3((T / 3 + 1 + 3) / 4), dim3(256), 0, s, T, n_ptr, capacity, ei, tile_range,
	                   big_tiles, flags);
	*elems_sorted = ei;
	*elems_free = eo;
}

}  // namespace bsr
