// The entropy codec for gfx950 (include/bloomscene_codec.h): interleaved rANS over a 16-bit integer model that is either
// evaluated per symbol from (mean, scale, Q) -- no cdf table -- or read from a caller's table.  The model is a template
// parameter of the SAME kernels, and one device function, model_c, gives c(j) to the encoder and the decoder alike.
//
//   k_codec_range     Gaussian model: k = rint(x / Q) of every kept element, the refusals, min and max (integer atomics)
//   k_codec_table     table model: the rows' monotonicity, the symbols' range; min = 0, max = L - 1
//   k_codec_encode    one wave a chunk of 64 T elements, steps in reverse: words to the END of the chunk's worst-case area
//   k_codec_offsets   one wave: the header and the exclusive scan of the chunks' sizes in chunk order, the stream's length
//   k_codec_pack      one workgroup a chunk: final states and words to their place in the stream
//   k_codec_decode    one wave a chunk, steps forward; the header, the offsets and every word read are checked
//
// LANE MAPPING.  Step s of chunk c is the 64 consecutive elements from (c T + s) 64 on, lane l the l-th: the operand loads
// of a step are 64 consecutive floats of [n, C] rows read through their stride (consecutive within a row, so a step touches
// one or two rows when C >= 64), and the decoder's stores are 64 consecutive floats.  A step's emitting lanes are found
// with one ballot; a lane's place among them is the count of set bits below it (v_mbcnt).
// DIVERGENCE.  The loops over chunks, steps and bisection trips are wave-uniform (T, L and the chunk count are); a lane
// past the end or skipped by `keep` sits a step out under a predicate.
// The kernels do integer work and two (encode) or ceil(log2 L) + 1 (decode) Phi evaluations a symbol: one division, one
// bsr_expf and five multiplications and additions each.
#include "common.h"
#include "../../include/bloomscene_codec.h"

namespace bsr {

#define BSR_CODEC_BLOCK 256            // four waves: four chunks
#define BSR_CODEC_MAX_BLOCKS 4096      // more chunks (or elements) than this covers: grid-stride
#define BSR_CODEC_HEAD 256             // bytes of the scratch before the per-chunk sections: min, -max
#define BSR_CODEC_UNSET 0x7f7f7f7f     // min and -max before the first element (a byte pattern: one memset)

struct CodecOperands {
	long long elements;        // n * C
	int C, r, Cw;              // Cw = C / r keep entries a row
	// Gaussian model
	const float *x, *mean, *scale, *q, *keep;
	long long xs, ms, ss;
	int q_mode;
	float scale_min;
	// table model
	const short* sym;
	const float* cdf;
	long long cs;
	int L;
};

// scratch: [0, 4) min, [4, 8) -max; from BSR_CODEC_HEAD one uint32 word count per chunk, then 64 uint32 states per chunk,
// then 64 T uint16 per chunk
struct CodecScratch {
	int* range;
	uint32_t* counts;
	uint32_t* states;
	uint16_t* words;
};

static long long codec_chunks(long long elements, int T)
{
	const long long per = 64LL * T;
	return (elements + per - 1) / per;
}
static size_t codec_counts_bytes(long long chunks) { return align_up((size_t)chunks * sizeof(uint32_t), 256); }
static CodecScratch codec_scratch(void* scratch, long long chunks)
{
	CodecScratch s;
	s.range = (int*)scratch;
	s.counts = (uint32_t*)((char*)scratch + BSR_CODEC_HEAD);
	s.states = (uint32_t*)((char*)s.counts + codec_counts_bytes(chunks));
	s.words = (uint16_t*)(s.states + chunks * 64);
	return s;
}
static long long codec_bound(long long elements, int T)
{
	const long long chunks = codec_chunks(elements, T);
	return BSR_CODEC_HEADER_BYTES + (chunks ? 4 * (chunks + 1) : 0) + 256 * chunks + 2 * elements;
}
// (the offsets are uint32: the worst case must stay below 2^32, which a small T at the largest counts does not)
static bool codec_supported(long long elements, int T)
{
	return elements >= 0 && elements <= BSR_CODEC_MAX_ELEMENTS && T >= 1 && T <= 65536 && codec_bound(elements, T) < (1LL << 32);
}
static unsigned codec_blocks(long long items)
{
	const long long b = (items + BSR_CODEC_BLOCK - 1) / BSR_CODEC_BLOCK;
	return (unsigned)(b < 1 ? 1 : (b < BSR_CODEC_MAX_BLOCKS ? b : BSR_CODEC_MAX_BLOCKS));
}

// Phi of the header, operation by operation (the unit is built with -ffp-contract=off)
__device__ __forceinline__ float codec_phi(float z)
{
	float a = fabsf(z) * 0.70710678118654752440f;
	a = a > 16.0f ? 16.0f : a;
	const float w = 0.3275911f * a;
	const float u = w / (1.0f + w);
	float p = -1.061405429f * u + 3.853875118f;
	p = p * u + -6.222859923f;
	p = p * u + 5.874886615f;
	p = p * u + -3.44449638f;
	p = p * u + 1.0f;
	const float h = 0.5f * (p * bsr_expf(-(a * a)));
	return z < 0.0f ? h : 1.0f - h;
}

__device__ __forceinline__ bool codec_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (false for a NaN)

// What a lane holds of its element: enough to evaluate c(j) for any j
template <int KIND> struct CodecElement;
template <> struct CodecElement<BSR_CODEC_KIND_GAUSSIAN> {
	float q, mean, s;
};
template <> struct CodecElement<BSR_CODEC_KIND_TABLE> {
	const float* row;
};

// c(j) of the header; kmin, L and Mf = float(65536 - 2 L) are wave-uniform.  Both directions call this and nothing else.
template <int KIND>
__device__ __forceinline__ uint32_t model_c(const CodecElement<KIND>& e, int j, int kmin, int L, float Mf)
{
	if (j <= 0) return 0u;
	if (j >= L) return 65536u;
	float P;
	if constexpr (KIND == BSR_CODEC_KIND_GAUSSIAN) {
		const float z = (((float)(kmin + j) - 0.5f) * e.q - e.mean) / e.s;
		P = codec_phi(z);
	} else {
		P = e.row[j];
	}
	return (uint32_t)(int)rintf(P * Mf) + 2u * (uint32_t)j;
}

__device__ __forceinline__ float codec_q(const CodecOperands& a, long long i, long long row)
{
	return a.q_mode == BSR_CODEC_Q_SINGLE ? a.q[0] : (a.q_mode == BSR_CODEC_Q_ROW ? a.q[row] : a.q[i]);
}
__device__ __forceinline__ bool codec_kept(const CodecOperands& a, long long row, int col)
{
	return !a.keep || a.keep[row * a.Cw + col / a.r] != 0.0f;
}

// Loads element i (< a.elements) of either model.  Returns whether it is coded (not skipped); status collects the
// refusals of the model's operands.
template <int KIND>
__device__ __forceinline__ bool codec_load(const CodecOperands& a, long long i, CodecElement<KIND>& e, float& qv, unsigned& status)
{
	if constexpr (KIND == BSR_CODEC_KIND_GAUSSIAN) {
		const long long row = i / a.C;
		const int col = (int)(i - row * a.C);
		if (!codec_kept(a, row, col)) return false;
		qv = codec_q(a, i, row);
		const float mv = a.mean[row * a.ms + col], sv = a.scale[row * a.ss + col];
		if (!(qv > 0.0f) || !codec_finite(qv)) status |= BSR_CODEC_BAD_STEP;
		if (!codec_finite(mv) || !codec_finite(sv)) status |= BSR_CODEC_BAD_MODEL;
		e.q = qv;
		e.mean = mv;
		e.s = sv < a.scale_min ? a.scale_min : sv;
	} else {
		e.row = a.cdf + i * a.cs;
		qv = 1.0f;
	}
	return true;
}

__device__ __forceinline__ int wave_min_int(int v)
{
	for (int o = 32; o > 0; o >>= 1) {
		const int w = __shfl_xor(v, o);
		v = w < v ? w : v;
	}
	return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v)
{
	for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
	return v;
}
__device__ __forceinline__ unsigned lanes_below(uint64_t m)   // set bits of m below this lane
{
	return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Gaussian model, first pass: range[0] = min k, range[1] = -max k over the kept elements, and the refusals.
__global__ void __launch_bounds__(BSR_CODEC_BLOCK) k_codec_range(CodecOperands a, int* __restrict__ range,
                                                                 unsigned* __restrict__ result)
{
	int lo = BSR_CODEC_UNSET, nhi = BSR_CODEC_UNSET;
	unsigned status = 0u;
	const long long stride = (long long)gridDim.x * BSR_CODEC_BLOCK;
	for (long long i = (long long)blockIdx.x * BSR_CODEC_BLOCK + threadIdx.x; i < a.elements; i += stride) {
		CodecElement<BSR_CODEC_KIND_GAUSSIAN> e;
		float qv;
		if (!codec_load<BSR_CODEC_KIND_GAUSSIAN>(a, i, e, qv, status)) continue;
		if (!(qv > 0.0f) || !codec_finite(qv)) continue;   // (refused above)
		const long long row = i / a.C;
		const float k = rintf(a.x[row * a.xs + (i - row * a.C)] / qv);
		if (!(fabsf(k) < 1073741824.0f)) {   // (a NaN fails it too)
			status |= BSR_CODEC_BAD_VALUE;
			continue;
		}
		const int ki = (int)k;
		lo = ki < lo ? ki : lo;
		nhi = -ki < nhi ? -ki : nhi;
	}
	lo = wave_min_int(lo);
	nhi = wave_min_int(nhi);
	status = wave_or(status);
	if ((threadIdx.x & 63) == 0) {
		if (lo != BSR_CODEC_UNSET) {
			atomicMin(&range[0], lo);
			atomicMin(&range[1], nhi);
		}
		if (status) atomicOr(&result[0], status);
	}
}

// Table model, first pass: every adjacent pair of every row, every symbol (encoder); the range is the caller's L.
__global__ void __launch_bounds__(BSR_CODEC_BLOCK) k_codec_table(CodecOperands a, long long rows, int* __restrict__ range,
                                                                 unsigned* __restrict__ result)
{
	unsigned status = 0u;
	const long long stride = (long long)gridDim.x * BSR_CODEC_BLOCK;
	const long long first = (long long)blockIdx.x * BSR_CODEC_BLOCK + threadIdx.x;
	for (long long i = first; i < rows * a.L; i += stride) {
		const long long row = i / a.L;
		const int j = (int)(i - row * a.L);
		const float lo = a.cdf[row * a.cs + j], hi = a.cdf[row * a.cs + j + 1];
		if (!(lo >= 0.0f && lo <= hi && hi <= 1.0f)) status |= BSR_CODEC_BAD_TABLE;   // (a NaN fails it)
	}
	if (a.sym)
		for (long long i = first; i < a.elements; i += stride)
			if (a.sym[i] < 0 || a.sym[i] >= a.L) status |= BSR_CODEC_BAD_SYMBOL;
	status = wave_or(status);
	if ((threadIdx.x & 63) == 0 && status) atomicOr(&result[0], status);
	if (range && first == 0 && a.elements > 0) {
		range[0] = 0;
		range[1] = -(a.L - 1);
	}
}

// (min, L) of what the first pass left; L = 0: nothing coded.  A span beyond int is reported as L = 2^31 - 1.
__device__ __forceinline__ void codec_span(const int* range, int& kmin, int& L)
{
	kmin = range[0];
	const int nhi = range[1];
	if (kmin == BSR_CODEC_UNSET) {
		kmin = 0;
		L = 0;
		return;
	}
	const long long span = -(long long)nhi - (long long)kmin + 1;
	L = span > 0x7fffffffLL ? 0x7fffffff : (int)span;
}

template <int KIND>
__global__ void __launch_bounds__(BSR_CODEC_BLOCK) k_codec_encode(CodecOperands a, int T, long long chunks, CodecScratch sc,
                                                                  const unsigned* __restrict__ result)
{
	int kmin, L;
	codec_span(sc.range, kmin, L);
	if (result[0] != 0u || L < 2 || L > BSR_CODEC_MAX_SYMBOLS) return;   // (uniform: k_codec_offsets writes a header-only stream)
	const float Mf = (float)(65536 - 2 * L);
	const int lane = threadIdx.x & 63;
	const long long per = 64LL * T;
	for (long long c = (long long)blockIdx.x * (BSR_CODEC_BLOCK / 64) + (threadIdx.x >> 6); c < chunks;
	     c += (long long)gridDim.x * (BSR_CODEC_BLOCK / 64)) {
		const long long base = c * per;
		const long long left = a.elements - base;
		const int steps = (int)(left >= per ? (long long)T : (left + 63) / 64);
		uint16_t* area = sc.words + base;
		uint32_t x = 1u << 16;
		uint32_t p = (uint32_t)per;   // the words so far are area[p, per)
		for (int s = steps - 1; s >= 0; s--) {
			const long long i = base + (long long)s * 64 + lane;
			bool act = i < a.elements;
			uint32_t b = 0u, f = 1u;
			if (act) {
				CodecElement<KIND> e;
				float qv;
				unsigned unused = 0u;
				act = codec_load<KIND>(a, i, e, qv, unused);
				if (act) {
					int j;
					if constexpr (KIND == BSR_CODEC_KIND_GAUSSIAN) {
						const long long row = i / a.C;
						j = (int)rintf(a.x[row * a.xs + (i - row * a.C)] / qv) - kmin;
					} else {
						j = (int)a.sym[i];
					}
					b = model_c<KIND>(e, j, kmin, L, Mf);
					f = model_c<KIND>(e, j + 1, kmin, L, Mf) - b;
				}
			}
			const bool emit = act && x >= (f << 16);   // (f <= 65535)
			const uint64_t m = wave_ballot(emit);
			p -= (uint32_t)__popcll(m);
			if (emit) {
				area[p + lanes_below(m)] = (uint16_t)(x & 0xffffu);
				x >>= 16;
			}
			if (act) x = ((x / f) << 16) + (x % f) + b;
		}
		sc.states[c * 64 + lane] = x;
		if (lane == 0) sc.counts[c] = (uint32_t)per - p;
	}
}

// One wave.  The header, the offsets (an exclusive scan in chunk order) and the length; the refusal of a span too wide.
__global__ void __launch_bounds__(64) k_codec_offsets(long long elements, int kind, int T, long long chunks, CodecScratch sc,
                                                      uint32_t* __restrict__ stream, unsigned* __restrict__ result)
{
	const int lane = threadIdx.x;
	int kmin, L;
	codec_span(sc.range, kmin, L);
	unsigned status = result[0];
	if (L > BSR_CODEC_MAX_SYMBOLS) status |= BSR_CODEC_BAD_SPAN;
	const bool coded = status == 0u && L >= 2;
	if (lane == 0) {
		stream[0] = BSR_CODEC_MAGIC;
		stream[1] = BSR_CODEC_FORMAT;
		stream[2] = (uint32_t)kind;
		stream[3] = (uint32_t)elements;
		stream[4] = (uint32_t)kmin;
		stream[5] = (uint32_t)L;
		stream[6] = (uint32_t)T;
		stream[7] = coded ? (uint32_t)chunks : 0u;
	}
	uint32_t length = BSR_CODEC_HEADER_BYTES;
	if (coded) {
		uint32_t* offsets = stream + BSR_CODEC_HEADER_BYTES / 4;
		uint32_t running = 0u;
		for (long long c0 = 0; c0 < chunks; c0 += 64) {
			const long long c = c0 + lane;
			const uint32_t bytes = c < chunks ? 256u + 2u * sc.counts[c] : 0u;
			const uint32_t incl = wave_inclusive_sum_dpp(bytes);
			if (c < chunks) offsets[c] = running + incl - bytes;
			running += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		}
		if (lane == 0) offsets[chunks] = running;
		length += 4u * (uint32_t)(chunks + 1) + running;
	}
	if (lane == 0) {
		result[0] = status;
		result[1] = status ? 0u : length;
	}
}

// One workgroup a chunk: 128 uint16 of final states, then the words, to offsets[c] behind the table.
__global__ void __launch_bounds__(BSR_CODEC_BLOCK) k_codec_pack(int T, long long chunks, CodecScratch sc,
                                                                uint16_t* __restrict__ stream)
{
	const uint32_t* header = (const uint32_t*)stream;
	if (header[7] == 0u) return;   // (uniform: header-only)
	const uint32_t* offsets = header + BSR_CODEC_HEADER_BYTES / 4;
	const long long per = 64LL * T;
	const size_t data = (BSR_CODEC_HEADER_BYTES + 4 * (size_t)(chunks + 1)) / 2;   // in uint16
	for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
		uint16_t* dst = stream + data + offsets[c] / 2;
		const uint16_t* st = (const uint16_t*)(sc.states + c * 64);
		if (threadIdx.x < 128) dst[threadIdx.x] = st[threadIdx.x];
		const uint32_t cnt = sc.counts[c];
		const uint16_t* src = sc.words + c * per + (per - cnt);
		for (uint32_t w = threadIdx.x; w < cnt; w += BSR_CODEC_BLOCK) dst[128 + w] = src[w];
	}
}

template <int KIND>
__device__ __forceinline__ void codec_store(float* out_f, short* out_s, long long i, int j, int kmin, float qv, bool coded)
{
	if constexpr (KIND == BSR_CODEC_KIND_GAUSSIAN) out_f[i] = coded ? (float)(j + kmin) * qv : 0.0f;
	else out_s[i] = (short)(coded ? j : 0);
}

template <int KIND>
__global__ void __launch_bounds__(BSR_CODEC_BLOCK) k_codec_decode(CodecOperands a, const uint32_t* __restrict__ stream,
                                                                  unsigned long long stream_bytes, float* __restrict__ out_f,
                                                                  short* __restrict__ out_s, unsigned* __restrict__ result)
{
	// the header, checked by every thread alike (uniform)
	unsigned status = result[1];   // (the table's check: written before this kernel, by nobody in it)
	uint32_t kmin_u = 0u, L_u = 0u, T_u = 1u, chunks_u = 0u;
	if (stream_bytes < BSR_CODEC_HEADER_BYTES) status |= BSR_CODEC_TRUNCATED;
	else {
		kmin_u = stream[4];
		L_u = stream[5];
		T_u = stream[6];
		chunks_u = stream[7];
		bool ok = stream[0] == BSR_CODEC_MAGIC && stream[1] == BSR_CODEC_FORMAT && stream[2] == (uint32_t)KIND &&
		          stream[3] == (uint32_t)a.elements && L_u <= BSR_CODEC_MAX_SYMBOLS && T_u >= 1u && T_u <= 65536u;
		if (ok) {
			const long long want = L_u >= 2u ? (a.elements + 64LL * T_u - 1) / (64LL * T_u) : 0;
			ok = (long long)chunks_u == want && (a.elements > 0 || L_u == 0u);
			if (KIND == BSR_CODEC_KIND_TABLE) ok = ok && (L_u == 0u ? a.elements == 0 : (int)L_u == a.L) && kmin_u == 0u;
			else ok = ok && (int)kmin_u > -(1 << 30) - 1 && (int)kmin_u < (1 << 30);
		}
		if (!ok) status |= BSR_CODEC_BAD_HEADER;
		else if (chunks_u && stream_bytes < BSR_CODEC_HEADER_BYTES + 4ull * (chunks_u + 1ull)) status |= BSR_CODEC_TRUNCATED;
	}
	const int kmin = (int)kmin_u, L = (int)L_u;
	const long long tid = (long long)blockIdx.x * BSR_CODEC_BLOCK + threadIdx.x;
	if (status != 0u || L < 2) {
		// nothing to read from the stream: zeros, or the one symbol of L == 1
		const long long stride = (long long)gridDim.x * BSR_CODEC_BLOCK;
		unsigned mine = 0u;
		for (long long i = tid; i < a.elements; i += stride) {
			CodecElement<KIND> e;
			float qv = 0.0f;
			const bool coded = status == 0u && L == 1 && codec_load<KIND>(a, i, e, qv, mine);
			codec_store<KIND>(out_f, out_s, i, 0, kmin, qv, coded);
		}
		status |= mine;
		if (tid == 0 && status) atomicOr(&result[0], status);
		else if (mine) atomicOr(&result[0], mine);
		return;
	}
	const long long chunks = chunks_u;
	const int T = (int)T_u;
	const uint32_t* offsets = stream + BSR_CODEC_HEADER_BYTES / 4;
	const unsigned long long data_bytes = stream_bytes - (BSR_CODEC_HEADER_BYTES + 4ull * (chunks_u + 1ull));
	const uint16_t* data = (const uint16_t*)(offsets + chunks + 1);
	const float Mf = (float)(65536 - 2 * L);
	int trips = 0;
	while ((1 << trips) < L) trips++;
	const int lane = threadIdx.x & 63;
	const long long per = 64LL * T;
	for (long long c = (long long)blockIdx.x * (BSR_CODEC_BLOCK / 64) + (threadIdx.x >> 6); c < chunks;
	     c += (long long)gridDim.x * (BSR_CODEC_BLOCK / 64)) {
		const long long base = c * per;
		const long long left = a.elements - base;
		const int steps = (int)(left >= per ? (long long)T : (left + 63) / 64);
		// the chunk's bytes: [off0, off1) of the data, 256 of states first
		const unsigned long long off0 = offsets[c], off1 = offsets[c + 1];
		uint32_t x = 1u << 16;
		uint32_t nwords = 0u;
		const uint16_t* words = data;
		if (off0 > off1 || (off0 & 1ull) || (off1 & 1ull) || off1 - off0 < 256ull) status |= BSR_CODEC_CORRUPT;
		else if (off1 > data_bytes) status |= BSR_CODEC_TRUNCATED;
		else {
			const uint16_t* st = data + off0 / 2;
			x = (uint32_t)st[2 * lane] | ((uint32_t)st[2 * lane + 1] << 16);
			words = st + 128;
			nwords = (uint32_t)((off1 - off0 - 256ull) / 2);
		}
		uint32_t next = 0u;   // words taken so far
		for (int s = 0; s < steps; s++) {
			const long long i = base + (long long)s * 64 + lane;
			const bool in = i < a.elements;
			CodecElement<KIND> e = {};
			float qv = 0.0f;
			const bool act = in && codec_load<KIND>(a, i, e, qv, status);
			const uint32_t v = x & 0xffffu;
			// c(lo) <= v < c(hi) throughout; the interval halves every trip and a trip at length 1 changes nothing
			int lo = 0, hi = L;
			uint32_t clo = 0u, chi = 65536u;
			for (int t = 0; t < trips; t++) {
				const int mid = (lo + hi) >> 1;
				const uint32_t cm = act ? model_c<KIND>(e, mid, kmin, L, Mf) : 0u;
				if (cm <= v) {
					lo = mid;
					clo = cm;
				} else {
					hi = mid;
					chi = cm;
				}
			}
			if (act) x = (chi - clo) * (x >> 16) + v - clo;
			const bool take = act && x < (1u << 16);
			const uint64_t m = wave_ballot(take);
			if (take) {
				const uint32_t at = next + lanes_below(m);
				uint32_t w = 0u;
				if (at < nwords) w = words[at];
				else status |= BSR_CODEC_TRUNCATED;
				x = (x << 16) | w;
			}
			next += (uint32_t)__popcll(m);
			if (in) codec_store<KIND>(out_f, out_s, i, lo, kmin, qv, act);
		}
		if (x != (1u << 16) || (lane == 0 && next != nwords)) status |= BSR_CODEC_CORRUPT;
	}
	status = wave_or(status);
	if (lane == 0 && status) atomicOr(&result[0], status);
}

// ---- host ----

static int codec_check_gaussian(const char* who, int n, int C, int r, const float* mean, long long ms, const float* scale,
                                long long ss, const float* q, int q_mode, const float* keep, float scale_min,
                                CodecOperands& a)
{
	if (n < 0 || C < 1 || r < 1 || C % r != 0) return fail("%s: need n >= 0, C >= 1, r >= 1 and C %% r == 0 (got %d, %d, %d)", who, n, C, r);
	if ((long long)n * C > BSR_CODEC_MAX_ELEMENTS) return fail("%s: n * C must be at most 2^30 (got %d * %d)", who, n, C);
	if (q_mode < BSR_CODEC_Q_SINGLE || q_mode > BSR_CODEC_Q_ELEMENT) return fail("%s: unknown q_mode %d", who, q_mode);
	if (!keep && r != 1) return fail("%s: r must be 1 without keep (got %d)", who, r);
	if (ms < C || ss < C) return fail("%s: row strides must be >= C = %d (got ms %lld, ss %lld)", who, C, ms, ss);
	if (!(scale_min > 0.0f) || !(scale_min < __builtin_inff())) return fail("%s: scale_min must be positive and finite", who);
	if (n > 0 && (!mean || !scale || !q)) return fail("%s: NULL mean, scale or q", who);
	if (((uintptr_t)mean | (uintptr_t)scale | (uintptr_t)q | (uintptr_t)keep) & 3) return fail("%s: mean, scale, q and keep must be 4-byte aligned", who);
	a = CodecOperands{};
	a.elements = (long long)n * C;
	a.C = C; a.r = r; a.Cw = C / r;
	a.mean = mean; a.scale = scale; a.q = q; a.keep = keep;
	a.ms = ms; a.ss = ss;
	a.q_mode = q_mode;
	a.scale_min = scale_min;
	return 0;
}

static int codec_check_table(const char* who, int n, int L, const float* cdf, long long cs, CodecOperands& a)
{
	if (n < 0 || (long long)n > BSR_CODEC_MAX_ELEMENTS) return fail("%s: n must be in [0, 2^30] (got %d)", who, n);
	if (L < 1 || L > BSR_CODEC_MAX_SYMBOLS) return fail("%s: L must be in [1, %d] (got %d)", who, BSR_CODEC_MAX_SYMBOLS, L);
	if (cs != 0 && cs < L + 1) return fail("%s: cs must be 0 (one row) or >= L + 1 = %d (got %lld)", who, L + 1, cs);
	if (n > 0 && !cdf) return fail("%s: NULL cdf", who);
	if ((uintptr_t)cdf & 3) return fail("%s: cdf must be 4-byte aligned", who);
	a = CodecOperands{};
	a.elements = n;
	a.C = 1; a.r = 1; a.Cw = 1;
	a.cdf = cdf;
	a.cs = cs;
	a.L = L;
	return 0;
}

static int codec_check_encode(const char* who, long long elements, int T, unsigned char* stream, size_t stream_bytes,
                              unsigned* result, void* scratch)
{
	if (T < 1 || T > 65536) return fail("%s: T must be in [1, 65536] (got %d)", who, T);
	if (!codec_supported(elements, T)) return fail("%s: %lld elements with T = %d would pass 2^32 bytes", who, elements, T);
	if (!stream || !result || !scratch) return fail("%s: NULL stream, result or scratch", who);
	if (stream_bytes < bsr_codec_stream_bound(elements, T))
		return fail("%s: stream_bytes %zu is below bsr_codec_stream_bound = %zu", who, stream_bytes, bsr_codec_stream_bound(elements, T));
	if (((uintptr_t)stream | (uintptr_t)result) & 3) return fail("%s: stream and result must be 4-byte aligned", who);
	if ((uintptr_t)scratch & 7) return fail("%s: scratch must be 8-byte aligned", who);
	return 0;
}

static int codec_check_decode(const char* who, const unsigned char* stream, const void* out, unsigned* result)
{
	if (!stream || !result) return fail("%s: NULL stream or result", who);
	if (((uintptr_t)stream | (uintptr_t)result) & 3) return fail("%s: stream and result must be 4-byte aligned", who);
	if ((uintptr_t)out & 3) return fail("%s: out must be 4-byte aligned", who);
	return 0;
}

template <int KIND>
static int codec_encode(const char* who, const CodecOperands& a, int T, unsigned char* stream, unsigned* result, void* scratch,
                        hipStream_t st)
{
	const long long chunks = codec_chunks(a.elements, T);
	const CodecScratch sc = codec_scratch(scratch, chunks);
	if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	if (hipMemsetAsync(sc.range, 0x7f, 2 * sizeof(int), st) != hipSuccess) return fail("%s: memset failed", who);
	if (a.elements > 0) {
		if (KIND == BSR_CODEC_KIND_GAUSSIAN)
			hipLaunchKernelGGL(k_codec_range, dim3(codec_blocks(a.elements)), dim3(BSR_CODEC_BLOCK), 0, st, a, sc.range, result);
		else {
			const long long rows = a.cs == 0 ? 1 : a.elements;
			const long long items = rows * a.L > a.elements ? rows * a.L : a.elements;
			hipLaunchKernelGGL(k_codec_table, dim3(codec_blocks(items)), dim3(BSR_CODEC_BLOCK), 0, st, a, rows, sc.range, result);
		}
		hipLaunchKernelGGL(k_codec_encode<KIND>, dim3(codec_blocks(chunks * 64)), dim3(BSR_CODEC_BLOCK), 0, st, a, T, chunks, sc,
		                   (const unsigned*)result);
	}
	hipLaunchKernelGGL(k_codec_offsets, dim3(1), dim3(64), 0, st, a.elements, KIND, T, chunks, sc, (uint32_t*)stream, result);
	if (a.elements > 0)
		hipLaunchKernelGGL(k_codec_pack, dim3((unsigned)(chunks < BSR_CODEC_MAX_BLOCKS ? chunks : BSR_CODEC_MAX_BLOCKS)),
		                   dim3(BSR_CODEC_BLOCK), 0, st, T, chunks, sc, (uint16_t*)stream);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

template <int KIND>
static int codec_decode(const char* who, const CodecOperands& a, const unsigned char* stream, size_t stream_bytes, float* out_f,
                        short* out_s, unsigned* result, hipStream_t st)
{
	if (hipMemsetAsync(result, 0, 2 * sizeof(unsigned), st) != hipSuccess) return fail("%s: memset failed", who);
	if (KIND == BSR_CODEC_KIND_TABLE && a.elements > 0) {
		const long long rows = a.cs == 0 ? 1 : a.elements;
		hipLaunchKernelGGL(k_codec_table, dim3(codec_blocks(rows * a.L)), dim3(BSR_CODEC_BLOCK), 0, st, a, rows, (int*)nullptr, result + 1);
	}
	// a wave a chunk of at least 64 elements (T >= 1): the grid covers the smallest T, larger ones leave waves idle
	hipLaunchKernelGGL(k_codec_decode<KIND>, dim3(codec_blocks(a.elements)), dim3(BSR_CODEC_BLOCK), 0, st, a,
	                   (const uint32_t*)stream, (unsigned long long)stream_bytes, out_f, out_s, result);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_codec_stream_bound(long long elements, int T)
{
	if (!codec_supported(elements, T)) return 0;
	return (size_t)codec_bound(elements, T);
}

size_t bsr_codec_scratch_bytes(long long elements, int T)
{
	if (!codec_supported(elements, T)) return 0;
	const long long chunks = codec_chunks(elements, T);
	return align_up(BSR_CODEC_HEAD + codec_counts_bytes(chunks) + (size_t)chunks * 256 + (size_t)chunks * 64 * T * 2, 256);
}

int bsr_codec_encode_gaussian(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                              const float* scale, long long ss, const float* q, int q_mode, const float* keep,
                              float scale_min, int T, unsigned char* stream, size_t stream_bytes, unsigned* result,
                              void* scratch, void* hip_stream)
{
	const char* who = "bsr_codec_encode_gaussian";
	CodecOperands a;
	if (codec_check_gaussian(who, n, C, r, mean, ms, scale, ss, q, q_mode, keep, scale_min, a)) return 1;
	if (xs < C) return fail("%s: row strides must be >= C = %d (got xs %lld)", who, C, xs);
	if (n > 0 && !x) return fail("%s: NULL x", who);
	if ((uintptr_t)x & 3) return fail("%s: x must be 4-byte aligned", who);
	if (codec_check_encode(who, a.elements, T, stream, stream_bytes, result, scratch)) return 1;
	a.x = x;
	a.xs = xs;
	return codec_encode<BSR_CODEC_KIND_GAUSSIAN>(who, a, T, stream, result, scratch, (hipStream_t)hip_stream);
}

int bsr_codec_decode_gaussian(int n, int C, int r, const unsigned char* stream, size_t stream_bytes, const float* mean,
                              long long ms, const float* scale, long long ss, const float* q, int q_mode,
                              const float* keep, float scale_min, float* out, unsigned* result, void* hip_stream)
{
	const char* who = "bsr_codec_decode_gaussian";
	CodecOperands a;
	if (codec_check_gaussian(who, n, C, r, mean, ms, scale, ss, q, q_mode, keep, scale_min, a)) return 1;
	if (codec_check_decode(who, stream, out, result)) return 1;
	if (n > 0 && !out) return fail("%s: NULL out", who);
	return codec_decode<BSR_CODEC_KIND_GAUSSIAN>(who, a, stream, stream_bytes, out, nullptr, result, (hipStream_t)hip_stream);
}

int bsr_codec_encode_table(int n, int L, const short* sym, const float* cdf, long long cs, int T, unsigned char* stream,
                           size_t stream_bytes, unsigned* result, void* scratch, void* hip_stream)
{
	const char* who = "bsr_codec_encode_table";
	CodecOperands a;
	if (codec_check_table(who, n, L, cdf, cs, a)) return 1;
	if (n > 0 && !sym) return fail("%s: NULL sym", who);
	if ((uintptr_t)sym & 1) return fail("%s: sym must be 2-byte aligned", who);
	if (codec_check_encode(who, a.elements, T, stream, stream_bytes, result, scratch)) return 1;
	a.sym = sym;
	return codec_encode<BSR_CODEC_KIND_TABLE>(who, a, T, stream, result, scratch, (hipStream_t)hip_stream);
}

int bsr_codec_decode_table(int n, int L, const unsigned char* stream, size_t stream_bytes, const float* cdf, long long cs,
                           short* out, unsigned* result, void* hip_stream)
{
	const char* who = "bsr_codec_decode_table";
	CodecOperands a;
	if (codec_check_table(who, n, L, cdf, cs, a)) return 1;
	if (!stream || !result) return fail("%s: NULL stream or result", who);
	if (((uintptr_t)stream | (uintptr_t)result) & 3) return fail("%s: stream and result must be 4-byte aligned", who);
	if (n > 0 && !out) return fail("%s: NULL out", who);
	if ((uintptr_t)out & 1) return fail("%s: out must be 2-byte aligned", who);
	return codec_decode<BSR_CODEC_KIND_TABLE>(who, a, stream, stream_bytes, nullptr, out, result, (hipStream_t)hip_stream);
}

}  // extern "C"
