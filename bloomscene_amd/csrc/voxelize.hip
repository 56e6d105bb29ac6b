// "Quantise points to a voxel lattice and keep each voxel once" for gfx950 (include/bloomscene_voxelize.h): np.unique of
// GaussianModel.voxelize_sample (scene/gaussian_model.py:435-438, "GM") and torch.round(...).int() + torch.unique(dim=0)
// of anchor_growing (GM:829-834).
//
//   k_voxel_init      the header words of the scratch: bounds = (INT_MAX, INT_MIN), invalid = 0
//   k_voxel_quantise  one row per thread and trip: fetch (coords / points through a stride / the composite of GM:824),
//                     quantise, q[e] = the coordinates; per-axis minimum and maximum and the invalid count go through
//                     the wave, then LDS, then ONE integer atomic per workgroup and word (a few thousand in all)
//   k_voxel_pack      key[e] = (x - xmin) << (by + bz) | (y - ymin) << bz | (z - zmin), payload[e] = e; workgroup 0
//                     writes the widths to the header and the status
//   k_voxel_hist / k_voxel_rowscan / k_voxel_scatter   one stable LSD radix pass on an 8-bit digit of the key, in the form
//                     of binning.hip's k_radix_* (digit-major histogram, 256 row scans (wg_scan.h), wave ballots for the in-round
//                     rank, stamped per-wave counters across the four waves).  Eight passes are enqueued; a pass whose
//                     digit lies above the key width returns at once, and the buffer that holds the result follows from
//                     the same header word -- the host never reads the width.
//   k_voxel_heads     per workgroup of 1024 sorted rows: the number of heads (key[i] != key[i - 1])
//   k_voxel_scan      ONE workgroup: exclusive scan of those numbers in order; U to the header and the status
//   k_voxel_emit      the heads again, ranked inside the workgroup with ballots: inverse[payload] = voxel; at a head
//                     first = payload (the sort is stable: the smallest position of the voxel), coords = the key
//                     unpacked, points = T(c) * T(s), start[voxel] = i
//   k_voxel_counts    counts[v] = start[v + 1] - start[v]
// WHY IT IS DETERMINISTIC.  Integer minimum, maximum and sum do not depend on the order of their operands; every other
// word is written by exactly one thread whose identity follows from the input alone.
#include "errors.h"
#include "wg_scan.h"
#include "../../include/bloomscene_voxelize.h"

namespace bsr {

#define BSR_VX_BLOCK 256
#define BSR_VX_WAVES (BSR_VX_BLOCK / 64)
#define BSR_VX_BINS 256
#define BSR_VX_QUANT_BLOCKS 2048     // the quantise kernel strides beyond this many workgroups
#define BSR_VX_SORT_BLOCKS 2048      // most workgroups (histogram columns) of a sort pass
#define BSR_VX_CHUNK_MIN 1024        // rows one sort workgroup owns, at least (a multiple of 256)
#define BSR_VX_CHUNK_TEST 64         // ... with BSR_VOXEL_FLAG_TEST_SMALL_CHUNK
#define BSR_VX_HEAD_ROWS 1024        // sorted rows per workgroup of k_voxel_heads / k_voxel_emit

// header words of the scratch (uint32; the bounds are ints)
enum { VX_MIN = 0, VX_MAX = 3, VX_INVALID = 6, VX_WIDTH = 7, VX_REFUSED = 8, VX_U = 9, VX_WORDS = 64 };

struct VoxelSource {
	int form, P, K;
	const void* src;
	long long src_stride;
	const float* anchor;
	const float* scaling;
	long long scaling_stride;
	const long long* rows;
};

__global__ void __launch_bounds__(64) k_voxel_init(uint32_t* __restrict__ hdr, uint32_t* __restrict__ invalid)
{
	const int t = threadIdx.x;
	if (hdr) hdr[t] = t < 3 ? 0x7fffffffu : (t < 6 ? 0x80000000u : 0u);
	if (invalid && t == 0) *invalid = 0u;
}

__device__ __forceinline__ float vx_rint(float x) { return __builtin_rintf(x); }
__device__ __forceinline__ double vx_rint(double x) { return __builtin_rint(x); }

// FORM: BSR_VOXEL_*; T: the points' type.  scale: T(s) (DIVIDE) or float(1.0 / s) (RECIPROCAL), formed on the host.
template <int FORM, typename T>
__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_quantise(int E, VoxelSource in, T scale, int rule,
                                                                 int* __restrict__ q, int* hdr, uint32_t* invalid)
{
	__shared__ int s_mn[3], s_mx[3];
	__shared__ uint32_t s_bad;
	const int tid = threadIdx.x, lane = tid & 63;
	if (tid < 3) {
		s_mn[tid] = 0x7fffffff;
		s_mx[tid] = (int)0x80000000;
	}
	if (tid == 0) s_bad = 0u;
	__syncthreads();
	int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
	int mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
	uint32_t bad = 0u;
	for (size_t e = (size_t)blockIdx.x * BSR_VX_BLOCK + tid; e < (size_t)E; e += (size_t)gridDim.x * BSR_VX_BLOCK) {
		const long long r = in.rows ? in.rows[e] : (long long)e;
		bool ok = r >= 0 && r < (long long)in.P;   // a row outside the source is never dereferenced
		int c[3] = {0, 0, 0};
		if (ok) {
			if (FORM == BSR_VOXEL_COORDS) {
				const int* p = (const int*)in.src + 3 * (size_t)r;
#pragma unroll
				for (int k = 0; k < 3; k++) c[k] = p[k];
			} else {
				T x[3];
				if (FORM == BSR_VOXEL_COMPOSITE) {
					const size_t a = (size_t)r / (size_t)in.K;
					const float* off = (const float*)in.src + 3 * (size_t)r;
#pragma unroll
					for (int k = 0; k < 3; k++) {
						const float prod = off[k] * in.scaling[a * (size_t)in.scaling_stride + k];   // (no contraction:
						x[k] = (T)(in.anchor[3 * a + k] + prod);                                    //  -ffp-contract=off)
					}
				} else {
					const T* p = (const T*)in.src + (size_t)r * (size_t)in.src_stride;
#pragma unroll
					for (int k = 0; k < 3; k++) x[k] = p[k];
				}
#pragma unroll
				for (int k = 0; k < 3; k++) {
					const T t = vx_rint(rule == BSR_VOXEL_RECIPROCAL ? x[k] * scale : x[k] / scale);
					const bool inside = t >= (T)-2147483648.0 && t < (T)2147483648.0;   // (false for NaN)
					ok = ok && inside;
					c[k] = inside ? (int)t : 0;
				}
			}
		}
		if (!ok) {
			c[0] = c[1] = c[2] = 0;
			bad++;
		} else {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				mn[k] = min(mn[k], c[k]);
				mx[k] = max(mx[k], c[k]);
			}
		}
#pragma unroll
		for (int k = 0; k < 3; k++) q[3 * e + k] = c[k];
	}
	if (!hdr && !invalid) return;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
		for (int k = 0; k < 3; k++) {
			mn[k] = min(mn[k], __shfl_xor(mn[k], d, 64));
			mx[k] = max(mx[k], __shfl_xor(mx[k], d, 64));
		}
		bad += __shfl_xor(bad, d, 64);
	}
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < 3; k++) {
			atomicMin(&s_mn[k], mn[k]);   // LDS
			atomicMax(&s_mx[k], mx[k]);
		}
		if (bad) atomicAdd(&s_bad, bad);
	}
	__syncthreads();
	if (hdr && tid < 3) {
		if (s_mn[tid] <= s_mx[tid]) {   // (this workgroup saw a valid row)
			atomicMin(&hdr[VX_MIN + tid], s_mn[tid]);
			atomicMax(&hdr[VX_MAX + tid], s_mx[tid]);
		}
	}
	if (tid == 0 && s_bad) {
		if (hdr) atomicAdd((uint32_t*)hdr + VX_INVALID, s_bad);
		if (invalid) atomicAdd(invalid, s_bad);
	}
}

// How the three coordinates share the 64-bit key: every thread derives it from the bounds in the header.
struct VoxelLayout {
	uint32_t mn[3], bits[3], width;
};
__device__ __forceinline__ VoxelLayout voxel_layout(const uint32_t* __restrict__ hdr)
{
	VoxelLayout L;
	L.width = 0u;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		L.mn[k] = hdr[VX_MIN + k];
		const uint32_t span = hdr[VX_MAX + k] - L.mn[k];   // max - min of two ints: below 2^32, exact modulo 2^32
		L.bits[k] = span ? 32u - (uint32_t)__clz(span) : 0u;
		L.width += L.bits[k];
	}
	return L;
}
__device__ __forceinline__ uint32_t vx_mask(uint32_t bits) { return bits >= 32u ? 0xffffffffu : ((1u << bits) - 1u); }

__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_pack(int E, const int* __restrict__ q, uint32_t* hdr,
                                                             uint64_t* __restrict__ keys, uint32_t* __restrict__ pay,
                                                             uint32_t* __restrict__ status)
{
	const uint32_t invalid = hdr[VX_INVALID];
	VoxelLayout L = voxel_layout(hdr);
	if (invalid) L.width = L.bits[0] = L.bits[1] = L.bits[2] = 0u;   // (the bounds may be the initial ones)
	const uint32_t refused = (invalid ? BSR_VOXEL_REFUSED_INVALID : 0u) | (L.width > 64u ? BSR_VOXEL_REFUSED_WIDE : 0u);
	const size_t e = (size_t)blockIdx.x * BSR_VX_BLOCK + threadIdx.x;
	// the words the later kernels read; no thread of this kernel reads them (every one derives the layout itself)
	if (e == 0) {
		hdr[VX_WIDTH] = refused ? 0u : L.width;
		hdr[VX_REFUSED] = refused;
		status[1] = invalid;
		status[2] = L.width;
		status[3] = refused;
		status[4] = L.bits[0];
		status[5] = L.bits[1];
		status[6] = L.bits[2];
		status[7] = 0u;
	}
	if (refused || e >= (size_t)E) return;
	const uint64_t dx = (uint32_t)q[3 * e] - L.mn[0], dy = (uint32_t)q[3 * e + 1] - L.mn[1], dz = (uint32_t)q[3 * e + 2] - L.mn[2];
	const uint32_t sx = L.bits[1] + L.bits[2];   // up to 64: then bx == 0 and dx == 0
	keys[e] = (sx < 64u ? dx << sx : 0ull) | (dy << L.bits[2]) | dz;   // (bz <= 32 and dy < 2^32: nothing is shifted out)
	pay[e] = (uint32_t)e;
}

// ---- stable LSD radix pass on bits [shift, shift + 8) of the key ----
// Workgroup b owns rows [b * chunk, (b + 1) * chunk).  hist is digit-major: hist[d * n_blocks + b].  Pass p reads buffer
// a when p is even: the passes below the key width run without a gap.
__device__ __forceinline__ bool vx_pass_active(const uint32_t* __restrict__ hdr, int shift)
{
	return (uint32_t)shift < hdr[VX_WIDTH];   // (0 when the call is refused)
}

__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_hist(int E, int chunk, int n_blocks, int shift,
                                                             const uint32_t* __restrict__ hdr,
                                                             const uint64_t* __restrict__ keys, uint32_t* __restrict__ hist)
{
	__shared__ uint32_t s_hist[BSR_VX_BINS];
	if (!vx_pass_active(hdr, shift)) return;
	const int tid = threadIdx.x;
	s_hist[tid] = 0u;
	__syncthreads();
	const size_t beg = (size_t)blockIdx.x * chunk, end = min((size_t)E, beg + chunk);
	for (size_t i = beg + tid; i < end; i += 4 * BSR_VX_BLOCK) {   // four loads in flight per trip
		uint64_t t[4];
#pragma unroll
		for (int k = 0; k < 4; k++) t[k] = (i + BSR_VX_BLOCK * k < end) ? keys[i + BSR_VX_BLOCK * k] : 0ull;
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (i + BSR_VX_BLOCK * k < end) atomicAdd(&s_hist[(uint32_t)(t[k] >> shift) & (BSR_VX_BINS - 1)], 1u);   // LDS
	}
	__syncthreads();
	hist[(size_t)tid * n_blocks + blockIdx.x] = s_hist[tid];
}

// One workgroup per digit d: exclusive scan of row d of the histogram (in place), 256 columns per step, and the row total.
__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_rowscan(int n_blocks, int shift, const uint32_t* __restrict__ hdr,
                                                                uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ digit_total)
{
	__shared__ uint32_t s_wave[2 * BSR_VX_WAVES];
	if (!vx_pass_active(hdr, shift)) return;
	const uint32_t total = wg_exclusive_scan<BSR_VX_WAVES, 1>(n_blocks, hist + (size_t)blockIdx.x * n_blocks, s_wave, true);
	if (threadIdx.x == 0) digit_total[blockIdx.x] = total;
}

__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_scatter(int E, int chunk, int n_blocks, int shift,
                                                                const uint32_t* __restrict__ hdr,
                                                                const uint64_t* __restrict__ keys_in,
                                                                const uint32_t* __restrict__ pay_in,
                                                                uint64_t* __restrict__ keys_out,
                                                                uint32_t* __restrict__ pay_out,
                                                                const uint32_t* __restrict__ hist,
                                                                const uint32_t* __restrict__ digit_total)
{
	__shared__ uint32_t s_off[BSR_VX_BINS];        // next output position per digit for this workgroup
	__shared__ uint32_t s_wcnt[4][BSR_VX_BINS];    // (round << 8 | count) per wave and digit, stamped
	__shared__ uint32_t s_scan[4];
	if (!vx_pass_active(hdr, shift)) return;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const size_t beg = (size_t)blockIdx.x * chunk, end = min((size_t)E, beg + chunk);
	const uint32_t row_prefix = hist[(size_t)tid * n_blocks + blockIdx.x];
	{   // digit base = exclusive scan of the 256 digit totals (thread d <-> digit d) + this workgroup's row prefix
		s_off[tid] = wg_exclusive_sum<BSR_VX_WAVES>(digit_total[tid], s_scan) + row_prefix;
	}
#pragma unroll
	for (int w = 0; w < 4; w++) s_wcnt[w][tid] = 0u;
	__syncthreads();
	const uint64_t lt = (1ull << lane) - 1ull;
	uint32_t round = 1u;   // (chunk <= 2^23 rows: the stamp fits its 24 bits)
	for (size_t base = beg; base < end; base += BSR_VX_BLOCK, round++) {
		const size_t i = base + tid;
		const bool valid = i < end;
		const uint64_t key = valid ? keys_in[i] : 0ull;
		const uint32_t p = valid ? pay_in[i] : 0u;
		const uint32_t d = (uint32_t)(key >> shift) & (BSR_VX_BINS - 1);
		// lanes of this wave with the same digit (invalid lanes match nobody)
		uint64_t peers = wave_ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const bool bit = (d >> b) & 1u;
			const uint64_t m = wave_ballot(bit);
			peers &= bit ? m : ~m;
		}
		const uint32_t rank_w = (uint32_t)__popcll(peers & lt);
		const uint32_t cnt_w = (uint32_t)__popcll(peers);
		if (valid && rank_w == 0) s_wcnt[wave][d] = (round << 8) | cnt_w;
		__syncthreads();
		if (valid) {
			uint32_t lower = 0u;
#pragma unroll
			for (int w = 0; w < 4; w++) {
				const uint32_t c = s_wcnt[w][d];
				if (w < wave && (c >> 8) == round) lower += c & 0xffu;
			}
			const uint32_t pos = s_off[d] + lower + rank_w;
			if (pos < (uint32_t)E) {   // (always: the histogram counted these very rows)
				keys_out[pos] = key;
				pay_out[pos] = p;
			}
		}
		__syncthreads();
		if (valid && rank_w == 0) atomicAdd(&s_off[d], cnt_w);   // LDS; order irrelevant, positions are taken
	}
}

// ---- heads, scan, emit ----
struct VoxelSorted {
	const uint64_t* keys;
	const uint32_t* pay;
};
// the buffer the last active pass wrote: a after an even number of passes
__device__ __forceinline__ VoxelSorted vx_sorted(const uint32_t* __restrict__ hdr, const uint64_t* ka, const uint32_t* pa,
                                                 const uint64_t* kb, const uint32_t* pb)
{
	const uint32_t passes = (hdr[VX_WIDTH] + 7u) >> 3;
	return (passes & 1u) ? VoxelSorted{kb, pb} : VoxelSorted{ka, pa};
}

__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_heads(int E, const uint32_t* __restrict__ hdr, const uint64_t* ka,
                                                              const uint32_t* pa, const uint64_t* kb, const uint32_t* pb,
                                                              uint32_t* __restrict__ block_heads)
{
	__shared__ uint32_t s_wave[BSR_VX_WAVES];
	if (hdr[VX_REFUSED]) return;
	const VoxelSorted S = vx_sorted(hdr, ka, pa, kb, pb);
	const int tid = threadIdx.x;
	uint32_t n = 0u;
#pragma unroll
	for (int k = 0; k < BSR_VX_HEAD_ROWS / BSR_VX_BLOCK; k++) {
		const size_t i = (size_t)blockIdx.x * BSR_VX_HEAD_ROWS + k * BSR_VX_BLOCK + tid;
		if (i < (size_t)E && (i == 0 || S.keys[i] != S.keys[i - 1])) n++;
	}
	const uint32_t heads = wg_total<BSR_VX_WAVES>(n, s_wave);
	if (tid == 0) block_heads[blockIdx.x] = heads;
}

// ONE workgroup of 1024: block_heads[0 .. n) -> exclusive prefixes in place, in order; U = the total.
__global__ void __launch_bounds__(1024) k_voxel_scan(int E, int n, uint32_t* hdr, uint32_t* __restrict__ block_heads,
                                                     uint32_t* __restrict__ start, uint32_t* __restrict__ status)
{
	__shared__ uint32_t s_wave[2 * 16];
	const int tid = threadIdx.x;
	if (hdr[VX_REFUSED]) {
		if (tid == 0) hdr[VX_U] = status[0] = 0u;
		return;
	}
	const uint32_t carry = wg_exclusive_scan<16, 1>(n, block_heads, s_wave, true);
	if (tid == 0) {
		hdr[VX_U] = status[0] = carry;
		start[carry] = (uint32_t)E;   // the end of the last voxel (start has 3 E >= E + 1 words)
	}
}

template <typename T>
__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_emit(int E, const uint32_t* __restrict__ hdr, const uint64_t* ka,
                                                             const uint32_t* pa, const uint64_t* kb, const uint32_t* pb,
                                                             const uint32_t* __restrict__ block_heads, T scale,
                                                             int* __restrict__ coords, long long* __restrict__ inverse,
                                                             long long* __restrict__ first, T* __restrict__ points,
                                                             uint32_t* __restrict__ start)
{
	__shared__ uint32_t s_wave[2][BSR_VX_WAVES];
	if (hdr[VX_REFUSED]) return;
	const VoxelSorted S = vx_sorted(hdr, ka, pa, kb, pb);
	const VoxelLayout L = voxel_layout(hdr);
	const int tid = threadIdx.x;
	uint32_t carry = block_heads[blockIdx.x];   // heads before this workgroup
	for (int k = 0; k < BSR_VX_HEAD_ROWS / BSR_VX_BLOCK; k++) {
		const size_t i = (size_t)blockIdx.x * BSR_VX_HEAD_ROWS + k * BSR_VX_BLOCK + tid;
		const bool valid = i < (size_t)E;
		const uint64_t key = valid ? S.keys[i] : 0ull;
		const bool head = valid && (i == 0 || key != S.keys[i - 1]);
		uint32_t total;
		const uint32_t before = wg_exclusive_count<BSR_VX_WAVES>(head, s_wave[k & 1], total);   // (set k & 1 was last read two barriers ago)
		if (valid) {
			// heads up to and including this row, minus one: row 0 is a head, so the number is never negative
			const uint32_t v = carry + before + (head ? 1u : 0u) - 1u;
			const uint32_t p = S.pay[i];
			inverse[p] = (long long)v;
			if (head) {
				first[v] = (long long)p;
				start[v] = (uint32_t)i;
				const uint32_t sx = L.bits[1] + L.bits[2];
				const uint32_t ux = sx < 64u ? (uint32_t)(key >> sx) : 0u;
				const uint32_t uy = (uint32_t)(key >> L.bits[2]) & vx_mask(L.bits[1]);   // (bz == 32: the high word)
				const uint32_t uz = (uint32_t)key & vx_mask(L.bits[2]);
				const int c[3] = {(int)(ux + L.mn[0]), (int)(uy + L.mn[1]), (int)(uz + L.mn[2])};
#pragma unroll
				for (int j = 0; j < 3; j++) coords[3 * (size_t)v + j] = c[j];
				if (points) {
#pragma unroll
					for (int j = 0; j < 3; j++) {
						const T x = (T)c[j] * scale;
						points[3 * (size_t)v + j] = c[j] == 0 ? (T)0 : x;   // a zero is +0 whatever the sign of s
					}
				}
			}
		}
		carry += total;
	}
}

__global__ void __launch_bounds__(BSR_VX_BLOCK) k_voxel_counts(const uint32_t* __restrict__ hdr,
                                                               const uint32_t* __restrict__ start,
                                                               long long* __restrict__ counts)
{
	if (hdr[VX_REFUSED]) return;
	const size_t v = (size_t)blockIdx.x * BSR_VX_BLOCK + threadIdx.x;
	if (v < (size_t)hdr[VX_U]) counts[v] = (long long)(start[v + 1] - start[v]);
}

// ---- host side ----

// The scratch of bsr_voxel_unique, laid out in one place.
struct VoxelScratch {
	size_t hdr, keys_a, keys_b, pay_a, pay_b, q, hist, digit_total, block_heads, bytes;
};
static int vx_sort_blocks_max(size_t E)   // histogram columns at the smallest chunk a call may ask for
{
	const size_t nb = (E + BSR_VX_CHUNK_TEST - 1) / BSR_VX_CHUNK_TEST;
	return (int)(nb < BSR_VX_SORT_BLOCKS ? nb : BSR_VX_SORT_BLOCKS);
}
static VoxelScratch voxel_scratch(size_t E)
{
	VoxelScratch s;
	size_t o = 0;
	s.hdr = o;          o += align_up(VX_WORDS * 4, 256);
	s.keys_a = o;       o += align_up(E * 8, 256);
	s.keys_b = o;       o += align_up(E * 8, 256);
	s.pay_a = o;        o += align_up(E * 4, 256);
	s.pay_b = o;        o += align_up(E * 4, 256);
	s.q = o;            o += align_up(E * 12, 256);   // the quantised rows; from k_voxel_scan on: start[U + 1]
	s.hist = o;         o += align_up((size_t)BSR_VX_BINS * vx_sort_blocks_max(E) * 4, 256);
	s.digit_total = o;  o += align_up(BSR_VX_BINS * 4, 256);
	s.block_heads = o;  o += align_up(((E + BSR_VX_HEAD_ROWS - 1) / BSR_VX_HEAD_ROWS) * 4, 256);
	s.bytes = o;
	return s;
}

// The checks both entry points make on the source; the scale the kernels use.
static int voxel_check_source(const char* who, int form, int rule, int E, int P, const void* src, long long src_stride,
                              const float* anchor, const float* scaling, long long scaling_stride, int K,
                              const long long* rows, double voxel_size, bool need_scale)
{
	if (form < BSR_VOXEL_COORDS || form > BSR_VOXEL_COMPOSITE) return fail("%s: unknown form %d", who, form);
	if (rule != BSR_VOXEL_DIVIDE && rule != BSR_VOXEL_RECIPROCAL) return fail("%s: unknown rule %d", who, rule);
	if (rule == BSR_VOXEL_RECIPROCAL && form == BSR_VOXEL_POINTS_D) return fail("%s: the reciprocal rule is fp32 only", who);
	if (E < 0 || P < 0) return fail("%s: need E >= 0 and P >= 0 (got %d, %d)", who, E, P);
	if (!rows && E != P) return fail("%s: without rows E must equal P (got %d, %d)", who, E, P);
	if (rows && form == BSR_VOXEL_COORDS) return fail("%s: the coordinate form takes no rows list", who);
	if (E == 0) return 0;
	if ((uintptr_t)rows & 7) return fail("%s: rows must be 8-byte aligned", who);
	if (P > 0 && !src) return fail("%s: NULL source", who);
	if ((uintptr_t)src & (form == BSR_VOXEL_POINTS_D ? 7 : 3)) return fail("%s: misaligned source", who);
	if ((form == BSR_VOXEL_POINTS_F || form == BSR_VOXEL_POINTS_D) && src_stride < 3)
		return fail("%s: src_stride must be >= 3 elements (got %lld)", who, src_stride);
	if (form == BSR_VOXEL_COMPOSITE) {
		if (K < 1 || P % K != 0) return fail("%s: P must be N * K with K >= 1 (got %d, %d)", who, P, K);
		if (P > 0 && (!anchor || !scaling)) return fail("%s: NULL anchor or scaling", who);
		if (((uintptr_t)anchor | (uintptr_t)scaling) & 3) return fail("%s: misaligned anchor or scaling", who);
		if (scaling_stride < 3) return fail("%s: scaling_stride must be >= 3 elements (got %lld)", who, scaling_stride);
	}
	if (need_scale && !(voxel_size == voxel_size && voxel_size != 0.0 && voxel_size - voxel_size == 0.0))
		return fail("%s: voxel_size must be finite and not 0 (got %g)", who, voxel_size);
	return 0;
}

static void launch_quantise(int form, int rule, int E, const VoxelSource& in, double voxel_size, int* q, int* hdr,
                            uint32_t* invalid, hipStream_t st)
{
	size_t nb = ((size_t)E + BSR_VX_BLOCK - 1) / BSR_VX_BLOCK;
	if (nb > BSR_VX_QUANT_BLOCKS) nb = BSR_VX_QUANT_BLOCKS;
	const dim3 grid((unsigned)nb), blk(BSR_VX_BLOCK);
	const float sf = (float)voxel_size;
	// torch's GPU rule: the reciprocal in double from the double scalar, rounded to fp32 once (1 / 0.001 -> 1000.0f)
	const float scale_f = rule == BSR_VOXEL_RECIPROCAL ? (float)(1.0 / voxel_size) : sf;
	switch (form) {
	case BSR_VOXEL_COORDS:
		hipLaunchKernelGGL((k_voxel_quantise<BSR_VOXEL_COORDS, float>), grid, blk, 0, st, E, in, scale_f, rule, q, hdr, invalid);
		break;
	case BSR_VOXEL_POINTS_F:
		hipLaunchKernelGGL((k_voxel_quantise<BSR_VOXEL_POINTS_F, float>), grid, blk, 0, st, E, in, scale_f, rule, q, hdr, invalid);
		break;
	case BSR_VOXEL_POINTS_D:
		hipLaunchKernelGGL((k_voxel_quantise<BSR_VOXEL_POINTS_D, double>), grid, blk, 0, st, E, in, voxel_size, rule, q, hdr, invalid);
		break;
	default:
		hipLaunchKernelGGL((k_voxel_quantise<BSR_VOXEL_COMPOSITE, float>), grid, blk, 0, st, E, in, scale_f, rule, q, hdr, invalid);
		break;
	}
}

}  // namespace bsr

using namespace bsr;

extern "C" {

int bsr_voxel_quantise(int form, int rule, int E, int P, const void* src, long long src_stride, const float* anchor,
                       const float* scaling, long long scaling_stride, int K, const long long* rows, double voxel_size,
                       int* q, unsigned int* invalid, void* stream)
{
	const char* who = "bsr_voxel_quantise";
	g_err[0] = 0;
	if (form == BSR_VOXEL_COORDS) return fail("%s: coordinates need no quantisation", who);
	if (voxel_check_source(who, form, rule, E, P, src, src_stride, anchor, scaling, scaling_stride, K, rows, voxel_size, true))
		return 1;
	if (E == 0) return 0;
	if (!q || ((uintptr_t)q & 3) || ((uintptr_t)invalid & 3)) return fail("%s: q must be a 4-byte aligned buffer", who);
	hipStream_t st = (hipStream_t)stream;
	const VoxelSource in{form, P, K, src, src_stride, anchor, scaling, scaling_stride, rows};
	if (invalid) hipLaunchKernelGGL(k_voxel_init, dim3(1), dim3(64), 0, st, (uint32_t*)nullptr, (uint32_t*)invalid);
	launch_quantise(form, rule, E, in, voxel_size, q, nullptr, (uint32_t*)invalid, st);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

size_t bsr_voxel_unique_scratch_bytes(int E)
{
	if (E <= 0) return 0;
	return voxel_scratch((size_t)E).bytes;
}

int bsr_voxel_unique(int form, int rule, int E, int P, const void* src, long long src_stride, const float* anchor,
                     const float* scaling, long long scaling_stride, int K, const long long* rows, double voxel_size,
                     int* coords, long long* inverse, long long* first, long long* counts, void* points,
                     unsigned int* status, void* scratch, unsigned int flags, void* stream)
{
	const char* who = "bsr_voxel_unique";
	g_err[0] = 0;
	const bool scaled = form != BSR_VOXEL_COORDS || points != nullptr;
	if (voxel_check_source(who, form, rule, E, P, src, src_stride, anchor, scaling, scaling_stride, K, rows, voxel_size, scaled))
		return 1;
	if (flags & ~BSR_VOXEL_FLAG_TEST_SMALL_CHUNK) return fail("%s: unknown flags 0x%x", who, flags);
	if (E == 0) return 0;
	if (!coords || !inverse || !first || !counts || !status || !scratch) return fail("%s: NULL buffer", who);
	if (((uintptr_t)coords | (uintptr_t)status) & 3) return fail("%s: coords and status must be 4-byte aligned", who);
	if (((uintptr_t)inverse | (uintptr_t)first | (uintptr_t)counts) & 7)
		return fail("%s: inverse, first and counts must be 8-byte aligned", who);
	if ((uintptr_t)points & (form == BSR_VOXEL_POINTS_D ? 7 : 3)) return fail("%s: misaligned points", who);
	if ((uintptr_t)scratch & 255) return fail("%s: scratch must be 256-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const VoxelScratch lay = voxel_scratch((size_t)E);
	char* base = (char*)scratch;
	uint32_t* hdr = (uint32_t*)(base + lay.hdr);
	uint64_t* ka = (uint64_t*)(base + lay.keys_a);
	uint64_t* kb = (uint64_t*)(base + lay.keys_b);
	uint32_t* pa = (uint32_t*)(base + lay.pay_a);
	uint32_t* pb = (uint32_t*)(base + lay.pay_b);
	int* q = (int*)(base + lay.q);
	uint32_t* hist = (uint32_t*)(base + lay.hist);
	uint32_t* digit_total = (uint32_t*)(base + lay.digit_total);
	uint32_t* block_heads = (uint32_t*)(base + lay.block_heads);
	const VoxelSource in{form, P, K, src, src_stride, anchor, scaling, scaling_stride, rows};
	const dim3 blk(BSR_VX_BLOCK);
	const unsigned row_blocks = (unsigned)(((size_t)E + BSR_VX_BLOCK - 1) / BSR_VX_BLOCK);

	hipLaunchKernelGGL(k_voxel_init, dim3(1), dim3(64), 0, st, hdr, (uint32_t*)nullptr);
	launch_quantise(form, rule, E, in, voxel_size, q, (int*)hdr, nullptr, st);
	hipLaunchKernelGGL(k_voxel_pack, dim3(row_blocks), blk, 0, st, E, (const int*)q, hdr, ka, pa, (uint32_t*)status);

	// rows per sort workgroup: a multiple of its granule, at most BSR_VX_SORT_BLOCKS workgroups
	const size_t granule = (flags & BSR_VOXEL_FLAG_TEST_SMALL_CHUNK) ? BSR_VX_CHUNK_TEST : BSR_VX_BLOCK;
	const size_t chunk_min = (flags & BSR_VOXEL_FLAG_TEST_SMALL_CHUNK) ? BSR_VX_CHUNK_TEST : BSR_VX_CHUNK_MIN;
	size_t chunk = (((size_t)E + BSR_VX_SORT_BLOCKS - 1) / BSR_VX_SORT_BLOCKS + granule - 1) / granule * granule;
	if (chunk < chunk_min) chunk = chunk_min;
	const int n_blocks = (int)(((size_t)E + chunk - 1) / chunk);   // <= vx_sort_blocks_max(E): the histogram fits
	for (int pass = 0; pass < 8; pass++) {
		const int shift = 8 * pass;
		const uint64_t* ki = (pass & 1) ? kb : ka;
		const uint32_t* pi = (pass & 1) ? pb : pa;
		uint64_t* ko = (pass & 1) ? ka : kb;
		uint32_t* po = (pass & 1) ? pa : pb;
		hipLaunchKernelGGL(k_voxel_hist, dim3(n_blocks), blk, 0, st, E, (int)chunk, n_blocks, shift, (const uint32_t*)hdr, ki, hist);
		hipLaunchKernelGGL(k_voxel_rowscan, dim3(BSR_VX_BINS), blk, 0, st, n_blocks, shift, (const uint32_t*)hdr, hist, digit_total);
		hipLaunchKernelGGL(k_voxel_scatter, dim3(n_blocks), blk, 0, st, E, (int)chunk, n_blocks, shift, (const uint32_t*)hdr, ki, pi,
		                   ko, po, (const uint32_t*)hist, (const uint32_t*)digit_total);
	}

	const unsigned head_blocks = (unsigned)(((size_t)E + BSR_VX_HEAD_ROWS - 1) / BSR_VX_HEAD_ROWS);
	uint32_t* start = (uint32_t*)q;   // (the quantised rows are in the keys now)
	hipLaunchKernelGGL(k_voxel_heads, dim3(head_blocks), blk, 0, st, E, (const uint32_t*)hdr, (const uint64_t*)ka,
	                   (const uint32_t*)pa, (const uint64_t*)kb, (const uint32_t*)pb, block_heads);
	hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(1024), 0, st, E, (int)head_blocks, hdr, block_heads, start, (uint32_t*)status);
	if (form == BSR_VOXEL_POINTS_D)
		hipLaunchKernelGGL(k_voxel_emit<double>, dim3(head_blocks), blk, 0, st, E, (const uint32_t*)hdr, (const uint64_t*)ka,
		                   (const uint32_t*)pa, (const uint64_t*)kb, (const uint32_t*)pb, (const uint32_t*)block_heads,
		                   voxel_size, coords, inverse, first, (double*)points, start);
	else
		hipLaunchKernelGGL(k_voxel_emit<float>, dim3(head_blocks), blk, 0, st, E, (const uint32_t*)hdr, (const uint64_t*)ka,
		                   (const uint32_t*)pa, (const uint64_t*)kb, (const uint32_t*)pb, (const uint32_t*)block_heads,
		                   (float)voxel_size, coords, inverse, first, (float*)points, start);
	hipLaunchKernelGGL(k_voxel_counts, dim3(row_blocks), blk, 0, st, (const uint32_t*)hdr, (const uint32_t*)start, counts);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
