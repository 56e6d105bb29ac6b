// The anchor position coder for gfx950 (include/bloomscene_anchor_codec.h): the 48-bit lattice keys of the anchors, sorted
// by the caller, their gaps coded with a per-chunk Golomb-Rice rule, 256 keys a chunk.
//
//   k_anchor_keys      a thread a row: the three lattice indices (anchor_lattice.h: rule A of bloomscene_anchor_state.h,
//                      the same device function) packed x << 32 | y << 16 | z; the refusals of the coordinates
//   k_anchor_lengths   a workgroup a chunk, a thread a key: the order and range of the keys, the chunk's k, each gap's
//                      code length, their sum over the workgroup (wg_scan.h) -> the chunk's bytes into the scratch
//   k_anchor_offsets   one workgroup: the header, the exclusive scan of the chunks' bytes in chunk order (wg_scan.h: a fixed
//                      order) into the offset table, the stream's length
//   k_anchor_write     a workgroup a chunk: the same codes again, each at its exclusive bit offset; the chunk's words are
//                      staged in LDS, where a lane ORs its code in with integer atomics (a word is shared by the codes
//                      that meet in it; OR is order-independent), then stored as consecutive words
//   k_anchor_decode    a wave a chunk, four chunks a workgroup: the chunk's words into LDS (consecutive loads), lane 0
//                      walks the codes one after the other (a code's place depends on every code before it) and leaves
//                      the gaps in LDS, then the 64 lanes add them up (a 64-bit wave scan, four rounds) and write the keys
//                      and the anchors
// The length pass and the write pass call ONE function for a thread's code (ac_thread_code), so the offsets and the words
// agree by construction.  The decoder reads a chunk's words through ac_peek alone, which gives zero bits beyond the chunk's
// end; every length is compared with the chunk's bit count before the position moves.
// DIVERGENCE.  Everything but the decoder's walk is a thread per key under a predicate.  The walk runs on one lane while 63
// idle: 255 short trips a chunk, the chunks of a scene side by side on the SIMDs (100 000 anchors are 391 waves).
#include "common.h"
#include "wg_scan.h"
#include "anchor_lattice.h"
#include "../../include/bloomscene_anchor_codec.h"

namespace bsr {

#define AC_BLOCK 256
#define AC_WAVES (AC_BLOCK / 64)
#define AC_B BSR_ANCHOR_CODEC_CHUNK
#define AC_WORDS (BSR_ANCHOR_CODEC_CHUNK_BYTES / 4)   // a chunk's most: 2 of the first key and k, 638 of gap bits
#define AC_HEADER_WORDS (BSR_ANCHOR_CODEC_HEADER_BYTES / 4)
#define AC_KEY_MASK 0xffffffffffffull
#define AC_MAX_K 47u
static_assert(AC_B == AC_BLOCK, "a thread a key of the chunk");
static_assert(AC_WORDS * 32 >= 64 + (AC_B - 1) * 80, "the staged words hold the longest chunk");

__device__ __forceinline__ bool ac_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (false for a NaN)

__global__ void __launch_bounds__(AC_BLOCK) k_anchor_keys(int N, int n, const float* __restrict__ anchor, size_t stride,
                                                          const float* __restrict__ bmin, const float* __restrict__ bmax,
                                                          const long long* __restrict__ rows,
                                                          unsigned long long* __restrict__ keys, unsigned* __restrict__ result)
{
	const long long i = (long long)blockIdx.x * AC_BLOCK + threadIdx.x;
	if (i >= (long long)n) return;
	const long long r = rows ? rows[i] : i;
	unsigned status = 0u;
	uint64_t key = 0ull;
	if (r < 0 || r >= (long long)N) status = BSR_ANCHOR_CODEC_BAD_ROW;
	else {
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const float x = anchor[(size_t)r * stride + c], lo = bmin[c];
			const float interval = anchor_interval(lo, bmax[c]);
			const float q = anchor_lattice_index(x, lo, interval);
			const bool ok = ac_finite(x) && ac_finite(lo) && ac_finite(interval) && q >= 0.0f && q <= 65535.0f;
			if (!ok) status = BSR_ANCHOR_CODEC_BAD_VALUE;
			key = (key << 16) | (uint64_t)(ok ? (uint32_t)q : 0u);
		}
	}
	keys[i] = status ? 0ull : key;
	if (status) atomicOr(&result[0], status);
}

// the rule's k for a chunk of m keys from `first` to `last`
__device__ __forceinline__ uint32_t ac_rice_k(uint64_t first, uint64_t last, int m)
{
	if (m < 2) return 0u;
	const uint64_t mean = (last - first) / (uint64_t)(m - 1);
	const uint32_t k = mean == 0ull ? 0u : 63u - (uint32_t)__clzll((long long)mean);
	return k < AC_MAX_K ? k : AC_MAX_K;   // (beyond 47 only for keys that are refused: the code stays within 80 bits)
}

struct AcCode {
	uint64_t lo, hi;   // the code's bits, lowest first
	uint32_t bits;     // 0: nothing is written
};

// the code of gap d under k: a prefix P of p bits (qh ones and a zero, or 32 ones), then w bits of V
__device__ __forceinline__ AcCode ac_code(uint64_t d, uint32_t k)
{
	d &= AC_KEY_MASK;   // (a gap of refused keys may be wider)
	const uint64_t qh = d >> k;
	uint32_t p, w;
	uint64_t P, V;
	if (qh < BSR_ANCHOR_CODEC_ESCAPE) {
		p = (uint32_t)qh + 1u; P = (1ull << qh) - 1ull; V = d & ((1ull << k) - 1ull); w = k;
	} else {
		p = BSR_ANCHOR_CODEC_ESCAPE; P = 0xffffffffull; V = d; w = 48u;
	}
	AcCode c;
	c.lo = P | (V << p);      // p is in [1, 32]
	c.hi = V >> (64u - p);
	c.bits = p + w;
	return c;
}

// Thread t's part of the chunk of m keys from keys[base]: the checks of its key, and the code of the gap before it (none
// for t == 0, whose key is written whole, and for t >= m).  k: the chunk's.
__device__ __forceinline__ AcCode ac_thread_code(const unsigned long long* __restrict__ keys, long long base, int m, int t,
                                                 uint32_t& k, unsigned& status)
{
	k = ac_rice_k(keys[base], keys[base + m - 1], m);
	AcCode code = {0ull, 0ull, 0u};
	if (t < m) {
		const uint64_t key = keys[base + t];
		if (key > AC_KEY_MASK) status |= BSR_ANCHOR_CODEC_BAD_KEY;
		if (base + t > 0) {
			const uint64_t prev = keys[base + t - 1];
			if (prev > key) status |= BSR_ANCHOR_CODEC_BAD_ORDER;
			if (t > 0) code = ac_code(key - prev, k);
		}
	}
	return code;
}

__device__ __forceinline__ int ac_chunk_keys(int n, long long base) { return (long long)n - base < AC_B ? (int)(n - base) : AC_B; }

__global__ void __launch_bounds__(AC_BLOCK) k_anchor_lengths(int n, const unsigned long long* __restrict__ keys,
                                                             uint32_t* __restrict__ sizes, unsigned* __restrict__ result)
{
	__shared__ uint32_t s_wave[AC_WAVES];
	const long long base = (long long)blockIdx.x * AC_B;
	uint32_t k;
	unsigned status = 0u;
	const AcCode code = ac_thread_code(keys, base, ac_chunk_keys(n, base), (int)threadIdx.x, k, status);
	const uint32_t total = wg_total<AC_WAVES>(code.bits, s_wave);
	if (threadIdx.x == 0) sizes[blockIdx.x] = 8u + 4u * ((total + 31u) >> 5);
	if (status) atomicOr(&result[0], status);
}

// One workgroup.  sizes: the chunks' bytes, scanned in place.
__global__ void __launch_bounds__(AC_BLOCK) k_anchor_offsets(int n, int chunks, const float* __restrict__ bmin,
                                                             const float* __restrict__ bmax, uint32_t* sizes,
                                                             uint32_t* __restrict__ stream, unsigned* result)
{
	__shared__ uint32_t s_wave[2 * AC_WAVES];
	const int t = threadIdx.x;
	// (one value a thread and step: thread t reads back below what thread t wrote)
	const uint32_t total = wg_exclusive_scan<AC_WAVES, 1>(chunks, sizes, s_wave, true);
	uint32_t* offsets = stream + AC_HEADER_WORDS;
	for (int c = t; c < chunks; c += AC_BLOCK) offsets[c] = sizes[c];
	if (t == 0) {
		unsigned status = result[0];
		stream[0] = BSR_ANCHOR_CODEC_MAGIC;
		stream[1] = BSR_ANCHOR_CODEC_FORMAT;
		stream[2] = (uint32_t)n;
		stream[3] = (uint32_t)chunks;
		stream[4] = AC_B;
		stream[5] = BSR_ANCHOR_CODEC_ESCAPE;
		for (int c = 0; c < 3; c++) {
			stream[6 + c] = __float_as_uint(bmin[c]);
			stream[9 + c] = __float_as_uint(bmax[c]);
			if (!ac_finite(bmin[c]) || !ac_finite(bmax[c]) || !ac_finite(anchor_interval(bmin[c], bmax[c])))
				status |= BSR_ANCHOR_CODEC_BAD_VALUE;
		}
		uint32_t length = BSR_ANCHOR_CODEC_HEADER_BYTES;
		if (chunks > 0) {
			offsets[chunks] = total;
			length += 4u * (uint32_t)(chunks + 1) + total;
		}
		result[0] = status;
		result[1] = status ? 0u : length;
	}
}

__global__ void __launch_bounds__(AC_BLOCK) k_anchor_write(int n, int chunks, const unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ stream, const unsigned* __restrict__ result)
{
	__shared__ uint32_t s_words[AC_WORDS];
	__shared__ uint32_t s_wave[AC_WAVES];
	if (result[0] != 0u) return;   // (uniform: the stream is refused)
	const int t = threadIdx.x;
	const long long base = (long long)blockIdx.x * AC_B;
	for (int w = t; w < AC_WORDS; w += AC_BLOCK) s_words[w] = 0u;
	uint32_t k, total;
	unsigned unused = 0u;
	const AcCode code = ac_thread_code(keys, base, ac_chunk_keys(n, base), t, k, unused);
	const uint32_t pos = wg_exclusive_sum<AC_WAVES>(code.bits, s_wave, total);   // (its barrier lies behind the zeroing)
	if (t == 0) {
		const uint64_t first = keys[base];
		s_words[0] = (uint32_t)first;
		s_words[1] = (uint32_t)(first >> 32) | (k << 16);
	}
	if (code.bits) {
		const uint32_t b = 64u + pos, w0 = b >> 5, s = b & 31u;
		const uint64_t sl = code.lo << s, sh = (code.hi << s) | (s ? code.lo >> (64u - s) : 0ull);
		const uint32_t x[4] = {(uint32_t)sl, (uint32_t)(sl >> 32), (uint32_t)sh, (uint32_t)(sh >> 32)};
#pragma unroll
		for (int j = 0; j < 4; j++)
			if (x[j] != 0u && w0 + j < AC_WORDS) atomicOr(&s_words[w0 + j], x[j]);
	}
	__syncthreads();
	const uint32_t words = 2u + ((total + 31u) >> 5);   // (= the bytes k_anchor_lengths counted / 4: the same codes)
	const uint32_t* offsets = stream + AC_HEADER_WORDS;
	uint32_t* dst = stream + AC_HEADER_WORDS + (chunks + 1) + offsets[blockIdx.x] / 4u;
	for (uint32_t w = t; w < words && w < AC_WORDS; w += AC_BLOCK) dst[w] = s_words[w];
}

// 64 bits of the nwords words at w from bit `pos` on, lowest first; zero bits beyond the last word
__device__ __forceinline__ uint64_t ac_peek(const uint32_t* w, uint32_t nwords, uint32_t pos)
{
	const uint32_t i = pos >> 5, s = pos & 31u;
	const uint64_t a = i < nwords ? w[i] : 0u, b = i + 1u < nwords ? w[i + 1u] : 0u, c = i + 2u < nwords ? w[i + 2u] : 0u;
	const uint64_t lo = a | (b << 32);
	return s ? (lo >> s) | (c << (64u - s)) : lo;
}

__device__ __forceinline__ uint64_t wave_inclusive_sum_u64(uint64_t x, int lane)
{
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint64_t y = __shfl_up((unsigned long long)x, (unsigned)o);
		if (lane >= o) x += y;
	}
	return x;
}

__global__ void __launch_bounds__(AC_BLOCK) k_anchor_decode(int n, const uint32_t* __restrict__ stream,
                                                            unsigned long long stream_bytes, float* __restrict__ anchor,
                                                            unsigned long long* __restrict__ keys_out,
                                                            float* __restrict__ bounds, unsigned* __restrict__ result)
{
	__shared__ uint32_t s_words[AC_WAVES][AC_WORDS];
	__shared__ uint64_t s_gaps[AC_WAVES][AC_B];
	__shared__ uint32_t s_walk[AC_WAVES][2];   // lane 0's status, and k
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// the header, checked by every thread alike (uniform over the grid)
	unsigned status = 0u;
	uint32_t chunks = 0u;
	float lo[3] = {0.0f, 0.0f, 0.0f}, interval[3] = {0.0f, 0.0f, 0.0f};
	if (stream_bytes < BSR_ANCHOR_CODEC_HEADER_BYTES) status = BSR_ANCHOR_CODEC_TRUNCATED;
	else {
		chunks = stream[3];
		bool ok = stream[0] == BSR_ANCHOR_CODEC_MAGIC && stream[1] == BSR_ANCHOR_CODEC_FORMAT && stream[2] == (uint32_t)n &&
		          chunks == ((uint32_t)n + AC_B - 1u) / AC_B && stream[4] == AC_B && stream[5] == BSR_ANCHOR_CODEC_ESCAPE;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			lo[c] = __uint_as_float(stream[6 + c]);
			const float hi = __uint_as_float(stream[9 + c]);
			interval[c] = anchor_interval(lo[c], hi);
			ok = ok && ac_finite(lo[c]) && ac_finite(hi) && ac_finite(interval[c]);
		}
		if (!ok) status = BSR_ANCHOR_CODEC_BAD_HEADER;
		else if (chunks > 0u && stream_bytes < BSR_ANCHOR_CODEC_HEADER_BYTES + 4ull * (chunks + 1ull)) status = BSR_ANCHOR_CODEC_TRUNCATED;
	}
	if (status) {
		if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&result[0], status);
		return;
	}
	if (bounds && blockIdx.x == 0 && threadIdx.x < 6) bounds[threadIdx.x] = __uint_as_float(stream[6 + threadIdx.x]);
	if (chunks == 0u) return;

	// ---- a wave a chunk: its words into LDS ----
	const uint32_t c = blockIdx.x * AC_WAVES + wave;
	const bool live = c < chunks;   // (uniform over the wave)
	const uint32_t* offsets = stream + AC_HEADER_WORDS;
	const unsigned long long data_bytes = stream_bytes - (BSR_ANCHOR_CODEC_HEADER_BYTES + 4ull * (chunks + 1ull));
	const uint32_t* data = offsets + chunks + 1u;
	const long long base = (long long)c * AC_B;
	int m = 0;
	uint32_t nw = 0u;      // the chunk's words; 0: the chunk is refused
	if (live) {
		m = ac_chunk_keys(n, base);
		const unsigned long long off0 = offsets[c], off1 = offsets[c + 1u];
		if (off0 > off1 || ((off0 | off1) & 3ull) || off1 - off0 < 8ull || off1 - off0 > BSR_ANCHOR_CODEC_CHUNK_BYTES ||
		    (c == 0u && off0 != 0ull))
			status |= BSR_ANCHOR_CODEC_CORRUPT;
		else if (off1 > data_bytes) status |= BSR_ANCHOR_CODEC_TRUNCATED;
		else {
			nw = (uint32_t)((off1 - off0) / 4ull);
			const uint32_t* src = data + off0 / 4ull;
			for (uint32_t w = lane; w < nw; w += 64u) s_words[wave][w] = src[w];
		}
	}
	__syncthreads();

	// ---- lane 0 walks the codes: gaps[0] is the first key, gaps[j] the gap before key j ----
	if (live && nw != 0u && lane == 0) {
		const uint32_t* w = s_words[wave];
		uint64_t* gaps = s_gaps[wave];
		const uint64_t head = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
		const uint32_t k = (uint32_t)(head >> 48);
		const uint32_t nbw = nw - 2u, nb = nbw * 32u;   // the gap bits' words and bits
		unsigned st = 0u;
		uint32_t pos = 0u;
		int j = 1;
		gaps[0] = head & AC_KEY_MASK;
		if (k > AC_MAX_K) st = BSR_ANCHOR_CODEC_CORRUPT;
		else {
			for (; j < m; j++) {
				const uint64_t v = ac_peek(w + 2, nbw, pos);
				const uint32_t ones = ~v == 0ull ? 64u : (uint32_t)__builtin_ctzll(~v);
				uint64_t d;
				uint32_t len;
				if (ones >= BSR_ANCHOR_CODEC_ESCAPE) {
					len = BSR_ANCHOR_CODEC_ESCAPE + 48u;
					if (pos + len > nb) break;
					d = ac_peek(w + 2, nbw, pos + BSR_ANCHOR_CODEC_ESCAPE) & AC_KEY_MASK;
					if ((d >> k) < BSR_ANCHOR_CODEC_ESCAPE) break;   // (an escape the rule does not call for)
				} else {
					len = ones + 1u + k;
					if (pos + len > nb) break;
					d = ((uint64_t)ones << k) | (ac_peek(w + 2, nbw, pos + ones + 1u) & ((1ull << k) - 1ull));
				}
				gaps[j] = d;
				pos += len;
			}
			if (j < m) st = BSR_ANCHOR_CODEC_CORRUPT;   // (a code past the chunk's end)
			else if (((pos + 31u) >> 5) != nbw) st = BSR_ANCHOR_CODEC_CORRUPT;   // (words that no code uses)
			else if ((pos & 31u) && (w[2u + (pos >> 5)] >> (pos & 31u)) != 0u) st = BSR_ANCHOR_CODEC_CORRUPT;   // (the padding)
		}
		for (; j < m; j++) gaps[j] = 0ull;
		s_walk[wave][0] = st;
		s_walk[wave][1] = k;
	}
	__syncthreads();

	// ---- the keys: first + the gaps up to each, 64 at a time; the anchors ----
	if (live) {
		const bool good = nw != 0u;
		if (good) status |= s_walk[wave][0];
		uint64_t carry = 0ull;
		for (int r = 0; r < AC_B / 64; r++) {
			const int j = r * 64 + lane;
			const uint64_t v = good && j < m ? s_gaps[wave][j] : 0ull;
			const uint64_t incl = wave_inclusive_sum_u64(v, lane);
			uint64_t key = carry + incl;
			carry += __shfl((unsigned long long)incl, 63);
			if (j < m) {
				if (key > AC_KEY_MASK) {
					status |= BSR_ANCHOR_CODEC_BAD_KEY;
					key &= AC_KEY_MASK;
				}
				const size_t i = (size_t)base + j;
				if (keys_out) keys_out[i] = key;
#pragma unroll
				for (int ch = 0; ch < 3; ch++)
					anchor[i * 3 + ch] = anchor_dequantise((float)(uint32_t)((key >> (32 - 16 * ch)) & 0xffffull), lo[ch], interval[ch]);
			}
		}
		// (carry is the last key: the chunk's k must be the one the rule gives)
		if (good && status == 0u && ac_rice_k(s_gaps[wave][0], carry, m) != s_walk[wave][1]) status |= BSR_ANCHOR_CODEC_CORRUPT;
		if (status) atomicOr(&result[0], status);
	}
}

static bool ac_supported(int n) { return n >= 0 && n <= BSR_ANCHOR_CODEC_MAX_N; }
static int ac_chunks(int n) { return (n + AC_B - 1) / AC_B; }

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_anchor_codec_stream_bound(int n)
{
	if (!ac_supported(n)) return 0;
	const size_t chunks = (size_t)ac_chunks(n);
	return BSR_ANCHOR_CODEC_HEADER_BYTES + (chunks ? 4 * (chunks + 1) : 0) + chunks * BSR_ANCHOR_CODEC_CHUNK_BYTES;
}

size_t bsr_anchor_codec_scratch_bytes(int n)
{
	if (!ac_supported(n)) return 0;
	return align_up((size_t)(ac_chunks(n) + 1) * sizeof(uint32_t), 256);
}

int bsr_anchor_keys(int N, int n, const float* anchor, long long anchor_stride, const float* bound_min, const float* bound_max,
                    const long long* rows, unsigned long long* keys, unsigned* result, void* hip_stream)
{
	const char* who = "bsr_anchor_keys";
	if (N < 0 || !ac_supported(n)) return fail("%s: need N >= 0 and n in [0, 2^27] (got N = %d, n = %d)", who, N, n);
	if (!rows && n > N) return fail("%s: n must be <= N without a row list (got n = %d, N = %d)", who, n, N);
	if (anchor_stride < 3) return fail("%s: anchor_stride must be >= 3 (got %lld)", who, anchor_stride);
	if (!result) return fail("%s: NULL result", who);
	if (n > 0 && (!anchor || !bound_min || !bound_max || !keys)) return fail("%s: NULL anchor, bounds or keys", who);
	if (((uintptr_t)anchor | (uintptr_t)bound_min | (uintptr_t)bound_max | (uintptr_t)result) & 3)
		return fail("%s: anchor, bounds and result must be 4-byte aligned", who);
	if (((uintptr_t)rows | (uintptr_t)keys) & 7) return fail("%s: rows and keys must be 8-byte aligned", who);
	hipStream_t st = (hipStream_t)hip_stream;
	if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	if (n > 0)
		hipLaunchKernelGGL(k_anchor_keys, dim3((unsigned)ac_chunks(n)), dim3(AC_BLOCK), 0, st, N, n, anchor, (size_t)anchor_stride,
		                   bound_min, bound_max, rows, keys, result);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_anchor_codec_encode(int n, const unsigned long long* keys, const float* bound_min, const float* bound_max,
                            unsigned char* stream, size_t stream_bytes, unsigned* result, void* scratch, void* hip_stream)
{
	const char* who = "bsr_anchor_codec_encode";
	if (!ac_supported(n)) return fail("%s: n must be in [0, 2^27] (got %d)", who, n);
	if (!bound_min || !bound_max || !stream || !result || !scratch) return fail("%s: NULL bounds, stream, result or scratch", who);
	if (n > 0 && !keys) return fail("%s: NULL keys", who);
	if (stream_bytes < bsr_anchor_codec_stream_bound(n))
		return fail("%s: stream_bytes %zu is below bsr_anchor_codec_stream_bound = %zu", who, stream_bytes, bsr_anchor_codec_stream_bound(n));
	if (((uintptr_t)bound_min | (uintptr_t)bound_max | (uintptr_t)stream | (uintptr_t)result | (uintptr_t)scratch) & 3)
		return fail("%s: bounds, stream, result and scratch must be 4-byte aligned", who);
	if ((uintptr_t)keys & 7) return fail("%s: keys must be 8-byte aligned", who);
	hipStream_t st = (hipStream_t)hip_stream;
	const int chunks = ac_chunks(n);
	uint32_t* sizes = (uint32_t*)scratch;
	if (chunks > 0)
		hipLaunchKernelGGL(k_anchor_lengths, dim3((unsigned)chunks), dim3(AC_BLOCK), 0, st, n, keys, sizes, result);
	hipLaunchKernelGGL(k_anchor_offsets, dim3(1), dim3(AC_BLOCK), 0, st, n, chunks, bound_min, bound_max, sizes, (uint32_t*)stream,
	                   result);
	if (chunks > 0)
		hipLaunchKernelGGL(k_anchor_write, dim3((unsigned)chunks), dim3(AC_BLOCK), 0, st, n, chunks, keys, (uint32_t*)stream,
		                   (const unsigned*)result);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_anchor_codec_decode(int n, const unsigned char* stream, size_t stream_bytes, float* anchor, unsigned long long* keys,
                            float* bounds, unsigned* result, void* hip_stream)
{
	const char* who = "bsr_anchor_codec_decode";
	if (!ac_supported(n)) return fail("%s: n must be in [0, 2^27] (got %d)", who, n);
	if (!result) return fail("%s: NULL result", who);
	if (stream_bytes > 0 && !stream) return fail("%s: NULL stream", who);
	if (n > 0 && !anchor) return fail("%s: NULL anchor", who);
	if (((uintptr_t)stream | (uintptr_t)anchor | (uintptr_t)bounds | (uintptr_t)result) & 3)
		return fail("%s: stream, anchor, bounds and result must be 4-byte aligned", who);
	if ((uintptr_t)keys & 7) return fail("%s: keys must be 8-byte aligned", who);
	hipStream_t st = (hipStream_t)hip_stream;
	if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	const int chunks = ac_chunks(n);
	const unsigned blocks = (unsigned)((chunks + AC_WAVES - 1) / AC_WAVES);
	hipLaunchKernelGGL(k_anchor_decode, dim3(blocks < 1u ? 1u : blocks), dim3(AC_BLOCK), 0, st, n, (const uint32_t*)stream,
	                   (unsigned long long)stream_bytes, anchor, keys, bounds, result);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
