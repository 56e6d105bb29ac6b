// Device-only sorting primitives of the per-tile depth sort (the kernels built from them: tile_sort.hip).
//
//   5. (binning.hip: steps 1-4) every tile's segment is sorted by its 64-bit key in LDS (a bucket-and-rank sort where
//      the depths spread, a bitonic network where they pile up: rank_sort and the sections above it), which yields
//      exactly the reference's stable-sort order because ids are unique within a tile -- so the
//      order in which step 2 drops equal-tile elements never reaches the output.
// Here: the swizzled round-based bitonic network, rank_sort, and the routines for segments of more than 1024 keys.
#pragma once
#include "common.h"

namespace bsr {

// What the placement passes (binning.hip) share with the sort: the radix digit and the size classes of the segments
#define BSR_RADIX_BITS 8
#define BSR_RADIX_BINS 256
#define BSR_SORT_SMALL_N 1024   // tiles with more instances go to the wide sort classes
#define BSR_SORT_SMALL BSR_SORT_SMALL_N
#define BSR_SORT_MID 2048       // (1024, 2048]: k_sort_tiles_mid where it is launched
#define BSR_SORT_CHUNK 4096     // up to here a segment is sorted in LDS; longer ones run hybrid in chunks of this size

// ---- per-tile bitonic sort of 64-bit keys ----
// Order = (tile, depth bits, Gaussian id) = the reference's stable radix-sort order (rasterizer_impl.cu:304-309): the
// tile part is done by the radix passes, here every tile's segment is sorted on the 64-bit key (depth bits, id).
// The network is the all-ascending form of bitonic sort (first step of every merge compares mirrored partners), so
// keys beyond n behave as +infinity pads.  Segments of up to 4096 keys are sorted in LDS by the round-based network
// below; longer ones (rare: a tile overlapped by > 4096 splats) run hybrid: every 4096-key chunk is sorted in LDS,
// then each merge does only its steps with partner distance >= 4096 in global memory (the plain steps right here)
// and finishes chunk by chunk in LDS.
#define BSR_PAD_KEY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ void cx(uint64_t& a, uint64_t& b)
{
	const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
	a = lo;
	b = hi;
}
__device__ __forceinline__ void cmp_exchange(uint64_t* k, int lo, int hi)
{
	const uint64_t a = k[lo], b = k[hi];
	if (a > b) { k[lo] = b; k[hi] = a; }
}
// global-memory steps of the hybrid (a compare-exchange whose upper index is >= n is the no-op a pad needs)
template <int NT>
__device__ __forceinline__ void merge_mirror_step(uint64_t* k, int n, int n2, int size, int tid)
{
	const int half = size >> 1, sh = __builtin_ctz(half);
	for (int i = tid; i < (n2 >> 1); i += NT) {
		const int blk = i >> sh, off = i & (half - 1);
		const int hi = blk * size + size - 1 - off;
		if (hi < n) cmp_exchange(k, blk * size + off, hi);
	}
}
template <int NT>
__device__ __forceinline__ void merge_stride_step(uint64_t* k, int n, int n2, int stride, int tid)
{
	for (int i = tid; i < (n2 >> 1); i += NT) {
		const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
		const int hi = lo | stride;
		if (hi < n) cmp_exchange(k, lo, hi);
	}
}

__device__ __forceinline__ uint64_t elem_key(const BinElem e) { return ((uint64_t)e.z << 32) | (uint64_t)e.y; }

// ---- round-based network: 2^M keys per thread, M network steps per LDS round trip --------------------------------
// A thread holds K = 2^M keys of a round in registers: the M index bits a round's steps act on enumerate the thread's
// keys, every other bit comes from the thread id, so M steps run between one read and one write of the keys (8 keys:
// 3 steps).  With n2 / K <= 64 (two trips per round up to 128) a whole segment belongs to ONE wave and needs no
// workgroup barrier at all: the small class sorts four tiles per workgroup, one per wave.  (Its predecessor ran two
// steps per barrier with 4 keys per thread, half of its 256 threads idle on a 512-key tile: 65 % of its wave-cycles
// were barrier and LDS-latency waits.)
// A merge of runs into runs of `size` = first round: the mirrored step + strides size/4 .. size/2^M (the thread's
// key set {i0 ^ a (size - 1) ^ sum c_b t_b} is closed under all of them), then rounds of up to M plain strides down
// to 1.  Keys in the mirrored half are labelled with complemented stride bits so that every plain step orders
// "bit clear below bit set" in both halves.
// LDS bank swizzle.  The keys are 8 bytes: a ds_read_b64 is served in two groups of 32 lanes, conflict-free when the
// 32 key slots differ mod 32; a ds_write_b64 in four groups of 16 lanes, slots mod 16.  With keys at their natural
// index the short strides are 2- to 4-way conflicts on every access (PMC on the predecessor: SQ_LDS_BANK_CONFLICT =
// 61 % of its LDS cycles).  Key i lives in slot i ^ ((i >> M) & 31): a bijection of [0, n2) for every power of two n2
// (bits are only folded downwards), found by enumerating XOR-linear maps against the access pattern of every round
// (M zero bits inserted into the thread index at any position), the load and the read-out: all conflict-free.  It is
// linear over XOR, so a thread swizzles ONE index per round and reaches its other keys by XOR with wave-uniform
// constants.
template <int M> __device__ __forceinline__ constexpr int swz_m(int i) { return i ^ ((i >> M) & 31); }

// Compare-exchange flavours.  F64: the keys of a segment whose depth bits all lie in [0x00100000, 0x7ff00000) are
// positive, normal, finite doubles when read as binary64, and for those the unsigned order of the bit patterns IS
// the numeric order: v_min_f64 / v_max_f64 return one operand unchanged each, two instructions instead of a 64-bit
// compare and four selects (selects and compares issue at 4.25 cycles on gfx950, the sort is bound by exactly these).
// The pad is +infinity (above every such key).  Segments holding any other depth pattern (NaN payloads, denormal or
// non-positive depths: the reference orders them by raw bits too) take the integer flavour.
#define BSR_PAD_F64 0x7FF0000000000000ull
template <bool F64>
__device__ __forceinline__ void cxt(uint64_t& a, uint64_t& b)
{
	if constexpr (F64) {
		double lo, hi;
		const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
		asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(x), "v"(y));
		asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(x), "v"(y));
		a = (uint64_t)__double_as_longlong(lo);
		b = (uint64_t)__double_as_longlong(hi);
	} else {
		cx(a, b);
	}
}
__device__ __forceinline__ bool key_is_plain_double(uint64_t k)
{
	const uint32_t h = (uint32_t)(k >> 32);
	return h >= 0x00100000u && h < 0x7ff00000u;
}

template <int M, int BIT, bool F64>
__device__ __forceinline__ void reg_step(uint64_t (&e)[1 << M])
{
#pragma unroll
	for (int c = 0; c < (1 << M); c++)
		if (!(c & (1 << BIT))) cxt<F64>(e[c], e[c | (1 << BIT)]);
}
// plain steps on local bits NS-1 .. 0
template <int M, int NS, bool F64>
__device__ __forceinline__ void reg_steps(uint64_t (&e)[1 << M])
{
	if constexpr (NS > 0) {
		reg_step<M, NS - 1, F64>(e);
		reg_steps<M, NS - 1, F64>(e);
	}
}
// mirrored step: local index (a, c), a = top bit: (0, c) <-> (1, ~c)
template <int M, bool F64>
__device__ __forceinline__ void reg_mirror(uint64_t (&e)[1 << M])
{
	constexpr int H = 1 << (M - 1);
#pragma unroll
	for (int c = 0; c < H; c++) cxt<F64>(e[c], e[H + (H - 1 - c)]);
}
// the K keys of a thread, ascending, entirely in registers (bitonic: sizes 2 .. K)
template <int M, bool F64>
__device__ __forceinline__ void reg_sort(uint64_t (&e)[1 << M])
{
#pragma unroll
	for (int sbit = 1; sbit <= M; sbit++) {
#pragma unroll
		for (int c = 0; c < (1 << M); c++)
			if (!(c & (1 << (sbit - 1)))) {
				const int partner = c ^ ((1 << sbit) - 1);
				cxt<F64>(e[c], e[partner]);
			}
#pragma unroll
		for (int b = sbit - 2; b >= 0; b--)
#pragma unroll
			for (int c = 0; c < (1 << M); c++)
				if (!(c & (1 << b))) cxt<F64>(e[c], e[c | (1 << b)]);
	}
}

// byte offset of local key L from the thread's first slot: XOR of the deltas of L's set bits (all wave-uniform)
template <int M>
__device__ __forceinline__ int local_delta(const int (&d)[M], int L)
{
	int x = 0;
#pragma unroll
	for (int b = 0; b < M; b++)
		if (L & (1 << b)) x ^= d[b];
	return x;
}
template <int M>
__device__ __forceinline__ void round_load(const char* lds, int p0, const int (&d)[M], uint64_t (&e)[1 << M])
{
#pragma unroll
	for (int L = 0; L < (1 << M); L++) e[L] = *reinterpret_cast<const uint64_t*>(lds + (p0 ^ local_delta<M>(d, L)));
}
template <int M>
__device__ __forceinline__ void round_store(char* lds, int p0, const int (&d)[M], const uint64_t (&e)[1 << M])
{
#pragma unroll
	for (int L = 0; L < (1 << M); L++) *reinterpret_cast<uint64_t*>(lds + (p0 ^ local_delta<M>(d, L))) = e[L];
}

template <bool BLOCK>
__device__ __forceinline__ void round_sync()
{
	if (BLOCK) {
		__syncthreads();
	} else {   // one wave owns the segment: its LDS operations execute in order; only the compiler must not reorder
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
}

// The plain strides 2^(rem-1) .. 1 of a merge, M per round, over n2 keys (slots swz_m<M>); t = thread index among
// the NT threads that share the segment.
template <int NT, int M, bool BLOCK, bool F64>
__device__ __forceinline__ void lds_stride_rounds(uint64_t* keys, int n2, int rem, int t)
{
	char* const lds = reinterpret_cast<char*>(keys);
	while (rem > 0) {
		const int ns = min(M, rem);
		const int lo = max(rem - M, 0);   // local bit b <-> index bit lo + b; a last, short round steps on bits ns-1 .. 0 only
		int d[M];
#pragma unroll
		for (int b = 0; b < M; b++) d[b] = swz_m<M>(1 << (lo + b)) << 3;
		round_sync<BLOCK>();
		for (int i = t; i < (n2 >> M); i += NT) {
			const int i0 = ((i >> lo) << (lo + M)) | (i & ((1 << lo) - 1));
			const int p0 = swz_m<M>(i0) << 3;
			uint64_t e[1 << M];
			round_load<M>(lds, p0, d, e);
			if (ns == M) reg_steps<M, M, F64>(e);
			else if (M > 3 && ns == 3) reg_steps<M, (M > 3 ? 3 : 1), F64>(e);
			else if (ns == 2) reg_steps<M, 2, F64>(e);
			else reg_steps<M, 1, F64>(e);
			round_store<M>(lds, p0, d, e);
		}
		rem -= ns;
	}
}

// Ascending sort of n2 (a power of two >= 2^M) keys in LDS whose aligned runs of 2^M are sorted already; pads
// (BSR_PAD_KEY) are ordinary keys.  Ends with a sync.  (Skipping the work items of blocks that hold pads only -- 20 % of
// the items of a 1200-key segment in 2048 slots -- was measured in round 6: no change in either sort kernel.)
template <int NT, int M, bool BLOCK, bool F64>
__device__ __forceinline__ void lds_sort_rounds(uint64_t* keys, int n2, int t)
{
	static_assert(M == 3 || M == 4, "8 or 16 keys per thread");
	char* const lds = reinterpret_cast<char*>(keys);
	for (int size = 2 << M; size <= n2; size <<= 1) {
		const int k = __builtin_ctz(size), lo = k - M, tlow = 1 << lo;
		// first round: mirror + strides size/4 .. size/2^M.  Local bits 0 .. M-2 <-> strides tlow << b; the top local
		// bit selects the mirrored half, whose keys carry complemented stride bits: its delta is (size - 1) ^ all strides
		int d[M], low_all = 0;
#pragma unroll
		for (int b = 0; b < M - 1; b++) {
			d[b] = swz_m<M>(tlow << b) << 3;
			low_all ^= tlow << b;
		}
		d[M - 1] = swz_m<M>((size - 1) ^ low_all) << 3;
		round_sync<BLOCK>();
		for (int i = t; i < (n2 >> M); i += NT) {
			const int i0 = ((i >> lo) << k) | (i & (tlow - 1));
			const int p0 = swz_m<M>(i0) << 3;
			uint64_t e[1 << M];
			round_load<M>(lds, p0, d, e);
			reg_mirror<M, F64>(e);
			reg_steps<M, M - 1, F64>(e);
			round_store<M>(lds, p0, d, e);
		}
		lds_stride_rounds<NT, M, BLOCK, F64>(keys, n2, k - M, t);
	}
	round_sync<BLOCK>();
}

// One segment of n <= n2 keys, sorted by the NT threads (thread index t) that share `keys` (n2 slots).  Runs of 2^M
// are sorted in registers on the way in (integer compare-exchange: the flavour of the merges is only known once every
// key has been seen) and the pads up to n2 are stored with them; returns this thread's vote on "every key I loaded is
// a positive, normal, finite binary64".
// Where a segment's unsorted keys come from: the binning elements (8- or 12-byte form), or plain 64-bit keys
// (k_bucket_sort stages its long tiles that way).  operator()(i) = key at global position i.
struct ElemKeys {
	const BinElem* __restrict__ elems;
	int compact;
	__device__ __forceinline__ uint64_t operator()(size_t i) const { return elem_key_m(elems, i, compact); }
};
struct RawKeys {
	const uint64_t* keys;   // (no __restrict__: k_bucket_sort writes the scratch it then sorts from)
	__device__ __forceinline__ uint64_t operator()(size_t i) const { return keys[i]; }
};
template <int NT, int M, typename Src>
__device__ __forceinline__ bool load_sorted_runs(uint64_t* keys, int n2, uint32_t start, int n, int t, const Src src)
{
	constexpr int K = 1 << M;
	bool plain = true;
	for (int i = t * K; i < n2; i += NT * K) {
		uint64_t e[K];
#pragma unroll
		for (int j = 0; j < K; j++) {
			e[j] = i + j < n ? src((size_t)start + (size_t)(i + j)) : BSR_PAD_KEY;
			plain = plain && (i + j >= n || key_is_plain_double(e[j]));
		}
		reg_sort<M, false>(e);
		const int p0 = swz_m<M>(i);   // i is a multiple of K: i + j == i ^ j
#pragma unroll
		for (int j = 0; j < K; j++) keys[p0 ^ swz_m<M>(j)] = e[j];
	}
	return plain;
}
template <int NT, int M, bool BLOCK, bool F64>
__device__ __forceinline__ void merge_loaded_runs(uint64_t* keys, int n2, uint32_t start, int n, int t,
                                                  uint32_t* __restrict__ point_list)
{
	if (F64) {   // the pads become +infinity (they sit at the ends of their runs either way)
		round_sync<BLOCK>();
		for (int i = n + t; i < n2; i += NT) keys[swz_m<M>(i)] = BSR_PAD_F64;
	}
	lds_sort_rounds<NT, M, BLOCK, F64>(keys, n2, t);
	for (int i = t; i < n; i += NT) point_list[start + i] = (uint32_t)keys[swz_m<M>(i)];
}

// ---- bucket-and-rank sort of one segment (round 6; the network above stays as the fall-back) -----------------------
// A segment's keys are (depth bits, id), and the depth bits of the splats over one tile spread over their range: instead
// of n log^2 n compare-exchanges the keys are dealt into NB = 2^NBLOG buckets by a MONOTONE map of the depth
// (common.h: rank_sort_bucket),
//     b = min(int((z - z_min) * (NB - 0.5) / (z_max - z_min)), NB - 1),
// (histogram with LDS atomics, one scan, one scatter: the keys then lie bucket by bucket, in arrival order inside a
// bucket), and a key's final place is its bucket's first position + the number of smaller keys in its bucket, counted
// against the bucket's members (keys are unique within a tile: ids are).  A key goes through LDS once (8-byte write,
// 8-byte read) plus ~2 reads per fellow member; the ids are written to point_list straight from the count.  The result is
// THE ascending order of the keys -- the same bits as the network's -- for every input; what depends on the input is
// only the price: a segment with a bucket of more than BSR_RANK_CAP keys (depths piled on one value), or with a depth
// word that is not a positive finite float (the reference orders those by raw bits too), is left untouched and the
// caller sorts it with the network.  Counters are 16 bits wide, two per dword (counts and offsets <= 4096): the
// low one cannot carry into the high one.
//   NT threads (t = index) share the segment; thread t holds keys i = t + NT q, q < KPT, in registers (valid: i < n) --
//   `out` (n slots of LDS) may therefore be the very area the keys were read from; cnt: NB / 2 dwords of LDS;
//   s_red (BLOCK only): 3 * NT / 64 dwords.  Ends without a sync: the caller syncs before `out` / `cnt` are reused.
#ifndef BSR_RANK_CAP
#define BSR_RANK_CAP 32
#endif
// maximum over the 64 lanes on the vector ALU (the steps of wave_inclusive_sum_dpp with max for +: lanes without a source
// take 0, the identity of an unsigned max; lane 63 ends with the total).  (Six __shfl_xor steps are six dependent
// ds_bpermute round trips: ~700 cycles per reduction, three reductions per sorted segment.)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));   // row_shr:1
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));   // row_shr:2
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));   // row_shr:4
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));   // row_shr:8
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
	x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
	return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
template <int NT, int KPT, int NBLOG, bool BLOCK>
__device__ __forceinline__ bool rank_sort(const uint64_t (&e)[KPT], int n, int t, uint64_t* out, uint32_t* cnt,
                                          uint32_t* s_red, uint32_t start, uint32_t* __restrict__ point_list)
{
	constexpr int NB = 1 << NBLOG, NDW = NB / 2, DPT = NDW / NT, NWV = NT / 64;
	static_assert(NDW % NT == 0 && DPT >= 1 && DPT <= 8, "the scan takes up to 8 counter dwords per thread");
	static_assert(KPT % 4 == 0, "the read-out takes four keys per thread and trip");
	const int lane = t & 63, wave = t >> 6;
	// ---- the range of the depth words
	uint32_t lo = 0xffffffffu, hi = 0u;
#pragma unroll
	for (int q = 0; q < KPT; q++)
		if (t + NT * q < n) {
			const uint32_t h = (uint32_t)(e[q] >> 32);
			lo = min(lo, h);
			hi = max(hi, h);
		}
	lo = ~wave_max_u32(~lo);
	hi = wave_max_u32(hi);
	if (BLOCK) {
		if (lane == 0) {
			s_red[wave] = lo;
			s_red[NWV + wave] = hi;
		}
		__syncthreads();
#pragma unroll
		for (int w = 0; w < NWV; w++) {
			lo = min(lo, s_red[w]);
			hi = max(hi, s_red[NWV + w]);
		}
	}
	if (lo == 0u || hi >= 0x7f800000u) return false;   // (uniform) not all positive finite floats: the network's integer flavour
	const float zlo = __uint_as_float(lo), scale = rank_sort_scale(zlo, __uint_as_float(hi), NB);
	// ---- histogram; the returning atomic also tells a key how many keys were in its bucket before it -- its place in the
	// bucket's run (one byte each: a count past 255 wraps, and such a segment is declined below)
#pragma unroll
	for (int w = 0; w < DPT; w++) cnt[t * DPT + w] = 0u;
	round_sync<BLOCK>();
	uint32_t arrival[KPT / 4];
#pragma unroll
	for (int q = 0; q < KPT / 4; q++) arrival[q] = 0u;
#pragma unroll
	for (int q = 0; q < KPT; q++)
		if (t + NT * q < n) {
			const uint32_t b = rank_sort_bucket(__uint_as_float((uint32_t)(e[q] >> 32)), zlo, scale, NB), sh = (b & 1u) << 4;
			const uint32_t before = (atomicAdd(&cnt[b >> 1], 1u << sh) >> sh) & 0xffu;   // LDS
			arrival[q >> 2] |= before << ((q & 3) << 3);
		}
	round_sync<BLOCK>();
	// ---- exclusive scan of the NB counts: thread t owns buckets 2 DPT t .. 2 DPT (t + 1) - 1
	uint32_t c[2 * DPT], total = 0u, cmax = 0u;
#pragma unroll
	for (int w = 0; w < DPT; w++) {
		const uint32_t v = cnt[t * DPT + w];
		c[2 * w] = v & 0xffffu;
		c[2 * w + 1] = v >> 16;
		total += c[2 * w] + c[2 * w + 1];
		cmax = max(cmax, max(c[2 * w], c[2 * w + 1]));
	}
	const uint32_t incl = wave_inclusive_sum_dpp(total);
	cmax = wave_max_u32(cmax);
	uint32_t run = incl - total;
	if (BLOCK) {
		if (lane == 63) s_red[2 * NWV + wave] = incl;
		__syncthreads();   // (also: every thread has read lo / hi above)
		if (lane == 0) s_red[wave] = cmax;
		for (int w = 0; w < wave; w++) run += s_red[2 * NWV + w];
		__syncthreads();
#pragma unroll
		for (int w = 0; w < NWV; w++) cmax = max(cmax, s_red[w]);
	}
	if (cmax > (uint32_t)BSR_RANK_CAP) return false;   // (uniform over the NT threads; nothing but cnt was written)
#pragma unroll
	for (int w = 0; w < DPT; w++) {
		const uint32_t o0 = run, o1 = run + c[2 * w];
		run = o1 + c[2 * w + 1];
		cnt[t * DPT + w] = o0 | (o1 << 16);
	}
	round_sync<BLOCK>();
	// ---- scatter: the keys bucket by bucket (every thread holds its keys in registers: `out` may be their old place)
	const uint16_t* const first = reinterpret_cast<const uint16_t*>(cnt);   // first position of every bucket
#pragma unroll
	for (int q = 0; q < KPT; q++)
		if (t + NT * q < n) {
			const uint32_t b = rank_sort_bucket(__uint_as_float((uint32_t)(e[q] >> 32)), zlo, scale, NB);
			out[(uint32_t)first[b] + ((arrival[q >> 2] >> ((q & 3) << 3)) & 0xffu)] = e[q];
		}
	round_sync<BLOCK>();
	// ---- a key's place = first position of its bucket + the number of smaller keys in the bucket
	constexpr int CHQ = 4;   // keys per thread and trip (all KPT at once: 5 KPT live registers)
#pragma unroll 1
	for (int q0 = 0; q0 < KPT && NT * q0 < n; q0 += CHQ) {
		uint64_t k[CHQ];
		uint32_t beg[CHQ], len[CHQ], rank[CHQ];
#pragma unroll
		for (int q = 0; q < CHQ; q++) {
			const int p = t + NT * (q0 + q);
			k[q] = 0ull;
			beg[q] = len[q] = rank[q] = 0u;
			if (p < n) {
				k[q] = out[p];
				const uint32_t b = rank_sort_bucket(__uint_as_float((uint32_t)(k[q] >> 32)), zlo, scale, NB);
				beg[q] = (uint32_t)first[b];
				const uint32_t end = b + 1u < (uint32_t)NB ? (uint32_t)first[b + 1u] : (uint32_t)n;
				len[q] = min(end - beg[q], (uint32_t)BSR_RANK_CAP);   // (<= the cap by the vote above: the clamp only bounds the
				                                                      // loop below whatever LDS holds)
			}
		}
		// JU members per key and trip: 4 JU independent LDS reads in flight (one member per trip left the loop at one
		// LDS round trip per member of the fullest bucket); the wave stops when its longest bucket is through
		uint32_t longest = max(max(len[0], len[1]), max(len[2], len[3]));
#ifndef BSR_RANK_JU_BLOCK
#define BSR_RANK_JU_BLOCK 2
#endif
		constexpr int JU = BLOCK ? BSR_RANK_JU_BLOCK : 4;   // (the workgroup-owned flavour runs in k_sort_tiles_wide's 80 VGPRs)
		for (uint32_t j0 = 0; wave_ballot(j0 < longest) != 0ull; j0 += JU) {
			uint64_t mem[CHQ][JU];
#pragma unroll
			for (int q = 0; q < CHQ; q++)
#pragma unroll
				for (int u = 0; u < JU; u++) mem[q][u] = out[min(beg[q] + j0 + u, (uint32_t)(n - 1))];   // (unconditional reads)
#pragma unroll
			for (int q = 0; q < CHQ; q++)
#pragma unroll
				for (int u = 0; u < JU; u++) rank[q] += (j0 + u < len[q] && mem[q][u] < k[q]) ? 1u : 0u;
		}
#pragma unroll
		for (int q = 0; q < CHQ; q++)
			if (t + NT * (q0 + q) < n) point_list[start + beg[q] + rank[q]] = (uint32_t)k[q];
	}
	return true;
}

// the same with the keys read from global memory (thread t: positions start + t + NT q, coalesced)
template <int NT, int KPT, int NBLOG, bool BLOCK, typename Src>
__device__ __forceinline__ bool rank_sort_from(const Src src, int n, int t, uint64_t* out, uint32_t* cnt, uint32_t* s_red,
                                               uint32_t start, uint32_t* __restrict__ point_list)
{
	uint64_t e[KPT];
#pragma unroll
	for (int q = 0; q < KPT; q++) e[q] = t + NT * q < n ? src((size_t)start + (size_t)(t + NT * q)) : 0ull;
	return rank_sort<NT, KPT, NBLOG, BLOCK>(e, n, t, out, cnt, s_red, start, point_list);
}

// Wave-owned segment: load, pick the compare-exchange flavour, sort.  No workgroup barrier anywhere.
template <int M>
__device__ __forceinline__ void sort_segment_wave(uint64_t* keys, int n2, uint32_t start, int n, int lane,
                                                  const BinElem* __restrict__ elems, uint32_t* __restrict__ point_list,
                                                  bool force_int, int compact)
{
	const bool plain = load_sorted_runs<64, M>(keys, n2, start, n, lane, ElemKeys{elems, compact}) && !force_int;
	if (wave_ballot(!plain) == 0ull)
		merge_loaded_runs<64, M, false, true>(keys, n2, start, n, lane, point_list);
	else
		merge_loaded_runs<64, M, false, false>(keys, n2, start, n, lane, point_list);
}

// Workgroup-owned segment (the wide classes): the same, with workgroup barriers and a workgroup vote.
template <int NT, int M, typename Src>
__device__ __forceinline__ void sort_segment_block(uint64_t* keys, int n2, uint32_t start, int n, int tid, const Src src,
                                                   uint32_t* __restrict__ point_list, bool force_int)
{
	const bool plain = load_sorted_runs<NT, M>(keys, n2, start, n, tid, src) && !force_int;
	if (__syncthreads_and(plain))
		merge_loaded_runs<NT, M, true, true>(keys, n2, start, n, tid, point_list);
	else
		merge_loaded_runs<NT, M, true, false>(keys, n2, start, n, tid, point_list);
}

// One long segment, 1024 < n <= BSR_SORT_CHUNK keys, sorted in `s_keys` (BSR_SORT_CHUNK slots) by the NT threads of
// the workgroup and read out to point_list[start ..).  Ends with a barrier (the keys are read out before the caller
// loads the next segment).
template <int NT, typename Src>
__device__ __forceinline__ void sort_long_tile_lds(uint64_t* s_keys, uint32_t* s_rank, uint32_t start, int n, int tid,
                                                   const Src src, uint32_t* __restrict__ point_list, int sort_mode)
{
	// bucket-and-rank sort first (sort_mode 0: 8 keys per thread = up to 8 NT keys, 4 NT buckets: s_rank holds 2 NT counter
	// dwords + the reduction words); declined segments go to the network
	if (sort_mode == 0) {
		constexpr int NBLOG = NT == 512 ? 11 : 10;
		static_assert(NT == 512 || NT == 256, "4096- or 2048-key segments");
		const bool done = rank_sort_from<NT, 8, NBLOG, true>(src, n, tid, s_keys, s_rank, s_rank + 2 * NT, start, point_list);
		__syncthreads();
		if (done) return;
	}
	int n2 = 1024;
	while (n2 < n) n2 <<= 1;
	sort_segment_block<NT, 3>(s_keys, n2, start, n, tid, src, point_list, (sort_mode & 1) != 0);
	__syncthreads();
}
// One segment of n > BSR_SORT_CHUNK keys, hybrid: every 4096-key chunk sorted in LDS into the global scratch k[0 .. n)
// (`src` may read that very scratch: a chunk is loaded completely before it is written back), the merge steps between
// chunks in global memory, the steps inside a chunk in LDS again.  Integer compare-exchange throughout (the global
// steps compare integers too).
template <int NT, typename Src>
__device__ __forceinline__ void sort_long_tile_hybrid(uint64_t* s_keys, uint64_t* k, uint32_t start, int n, int tid,
                                                      const Src src, uint32_t* __restrict__ point_list)
{
	constexpr int CH = BSR_SORT_CHUNK;
	int n2 = 1;
	while (n2 < n) n2 <<= 1;
	// runs of CH: every chunk sorted on its own in LDS
	for (int base = 0; base < n; base += CH) {
		const int m = min(CH, n - base);
		__syncthreads();
		load_sorted_runs<NT, 3>(s_keys, CH, start + (uint32_t)base, m, tid, src);
		lds_sort_rounds<NT, 3, true, false>(s_keys, CH, tid);
		for (int i = tid; i < m; i += NT) k[base + i] = s_keys[swz_m<3>(i)];
	}
	// merges of runs longer than CH: far partners in global memory, the rest per chunk in LDS
	for (int size = 2 * CH; size <= n2; size <<= 1) {
		__syncthreads();
		merge_mirror_step<NT>(k, n, n2, size, tid);
		for (int stride = size >> 2; stride >= CH; stride >>= 1) {
			__syncthreads();
			merge_stride_step<NT>(k, n, n2, stride, tid);
		}
		for (int base = 0; base < n; base += CH) {
			const int m = min(CH, n - base);
			__syncthreads();
			for (int i = tid; i < CH; i += NT) s_keys[swz_m<3>(i)] = i < m ? k[base + i] : BSR_PAD_KEY;
			lds_stride_rounds<NT, 3, true, false>(s_keys, CH, 12, tid);   // strides CH/2 .. 1
			__syncthreads();
			for (int i = tid; i < m; i += NT) k[base + i] = s_keys[swz_m<3>(i)];
		}
	}
	__syncthreads();
	for (int i = tid; i < n; i += NT) point_list[start + i] = (uint32_t)k[i];
	__syncthreads();
}

}  // namespace bsr
