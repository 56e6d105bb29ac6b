// GaussianModel.adjust_anchor for gfx950 (include/bloomscene_adjust.h): the decisions with their plan, and the one-pass
// prune + append of every per-anchor tensor.
//
//   k_decide_flags  a 256-thread workgroup owns one block of BSR_ADJUST_SCAN offsets (the first `blocks_o` workgroups) or
//                   anchors (the rest): the flag bytes, and the block's counts of om / of kept rows and am (wg_scan.h: wg_total)
//   k_decide_plan   a workgroup per block of anchors: the kept rows of the blocks before it (wg_scan.h: wg_total_of), the rank of
//                   each of its kept rows from wave ballots, src_of[rank] = row; workgroup 0 also adds up the status
//   k_rows_resize   the multi-tensor shape of adam.hip: the descriptors travel in the kernel-argument block and a
//                   workgroup finds its (tensor, chunk of BSR_RESIZE_CHUNK output elements) by a wave-uniform binary
//                   search of blockIdx.x.  A thread divides ONCE, the number of its first piece by the pieces of a row; the
//                   later pieces of the thread lie 256 further, which is a wave-uniform (rows, columns) step.  All source
//                   rows of a thread are read before its first load, all loads issued before its first store.
// Nothing here dereferences a src_of entry it has not compared with N first, and no thread writes outside
// [0, (n_keep + A) * width) of a dst.
#include "common.h"
#include "errors.h"
#include "wg_scan.h"
#include "../../include/bloomscene_adjust.h"

#include <cmath>

namespace bsr {

#define ADJ_BLOCK 256
#define ADJ_WAVES (ADJ_BLOCK / 64)
#define ADJ_SCAN BSR_ADJUST_SCAN
#define ADJ_ROUNDS (ADJ_SCAN / ADJ_BLOCK)

struct DecideScalars {
	float thr[BSR_ADJUST_MAX_LEVELS];
	int L;
	float offset_count_min, anchor_count_min, min_opacity;
};

__global__ void __launch_bounds__(ADJ_BLOCK) k_decide_flags(int N, int K, int blocks_o, const float* __restrict__ opacity_accum,
                                                            const float* __restrict__ anchor_demon,
                                                            const float* __restrict__ offset_gradient_accum,
                                                            const float* __restrict__ offset_denom, const DecideScalars s,
                                                            unsigned char* __restrict__ offset_flags,
                                                            unsigned char* __restrict__ anchor_flags,
                                                            uint32_t* __restrict__ keep_count, uint32_t* __restrict__ am_count,
                                                            uint32_t* __restrict__ om_count)
{
	__shared__ uint32_t part[2][ADJ_WAVES];
	if ((int)blockIdx.x < blocks_o) {   // (uniform over the workgroup)
		const long long total = (long long)N * K;
		uint32_t n_om = 0;
#pragma unroll
		for (int q = 0; q < ADJ_ROUNDS; q++) {
			const long long j = (long long)blockIdx.x * ADJ_SCAN + q * ADJ_BLOCK + threadIdx.x;
			bool om = false;
			if (j < total) {
				const float d = offset_denom[j];
				float g = offset_gradient_accum[j] / d;
				if (g != g) g = 0.0f;
				g = fabsf(g);
				om = d > s.offset_count_min;
				uint32_t f = 0;
				if (om) {
					f = BSR_ADJUST_OFFSET_VALID;
					for (int i = 0; i < s.L; i++)
						if (g >= s.thr[i]) f |= 1u << i;
				}
				offset_flags[j] = (unsigned char)f;
			}
			n_om += om ? 1u : 0u;
		}
		n_om = wg_total<ADJ_WAVES>(n_om, part[0]);
		if (threadIdx.x == 0) om_count[blockIdx.x] = n_om;
		return;
	}
	const int b = (int)blockIdx.x - blocks_o;
	uint32_t n_keep = 0, n_am = 0;
#pragma unroll
	for (int q = 0; q < ADJ_ROUNDS; q++) {
		const long long r = (long long)b * ADJ_SCAN + q * ADJ_BLOCK + threadIdx.x;
		bool keep = false, am = false;
		if (r < (long long)N) {
			const float a = opacity_accum[r], d = anchor_demon[r];
			am = d > s.anchor_count_min;
			const float bound = s.min_opacity * d;
			const bool prune = a < bound && am;
			keep = !prune;
			anchor_flags[r] = (unsigned char)((prune ? BSR_ADJUST_ANCHOR_PRUNE : 0) | (am ? BSR_ADJUST_ANCHOR_VALID : 0));
		}
		n_keep += keep ? 1u : 0u;
		n_am += am ? 1u : 0u;
	}
	n_keep = wg_total<ADJ_WAVES>(n_keep, part[0]);
	n_am = wg_total<ADJ_WAVES>(n_am, part[1]);
	if (threadIdx.x == 0) {
		keep_count[b] = n_keep;
		am_count[b] = n_am;
	}
}

__global__ void __launch_bounds__(ADJ_BLOCK) k_decide_plan(int N, int blocks_a, int blocks_o,
                                                           const unsigned char* __restrict__ anchor_flags,
                                                           const uint32_t* __restrict__ keep_count,
                                                           const uint32_t* __restrict__ am_count,
                                                           const uint32_t* __restrict__ om_count, int* __restrict__ src_of,
                                                           uint32_t* __restrict__ status)
{
	__shared__ uint32_t part[4][ADJ_WAVES];
	__shared__ uint32_t wave_count[ADJ_ROUNDS][ADJ_WAVES];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (blockIdx.x == 0) {
		const uint32_t kept = wg_total_of<ADJ_WAVES>(keep_count, blocks_a, part[1]);
		const uint32_t am = wg_total_of<ADJ_WAVES>(am_count, blocks_a, part[2]);
		const uint32_t om = wg_total_of<ADJ_WAVES>(om_count, blocks_o, part[3]);
		if (threadIdx.x == 0) {
			status[0] = kept;
			status[1] = am;
			status[2] = om;
			status[3] = 0;
		}
	}
	uint32_t rank = wg_total_of<ADJ_WAVES>(keep_count, (int)blockIdx.x, part[0]);   // of the first kept row of this block
	bool keep[ADJ_ROUNDS];
	uint32_t below[ADJ_ROUNDS];
#pragma unroll
	for (int q = 0; q < ADJ_ROUNDS; q++) {
		const long long r = (long long)blockIdx.x * ADJ_SCAN + q * ADJ_BLOCK + threadIdx.x;
		keep[q] = r < (long long)N && !(anchor_flags[r] & BSR_ADJUST_ANCHOR_PRUNE);
		const uint64_t votes = wave_ballot(keep[q]);
		below[q] = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
		if (lane == 0) wave_count[q][wave] = (uint32_t)__popcll(votes);
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < ADJ_ROUNDS; q++) {
		for (int w = 0; w < ADJ_WAVES; w++)
			if (w < wave) rank += wave_count[q][w];
		// rank + below < the number of kept rows <= N: inside src_of
		if (keep[q]) src_of[rank + below[q]] = (int)((long long)blockIdx.x * ADJ_SCAN + q * ADJ_BLOCK + threadIdx.x);
		for (int w = 0; w < ADJ_WAVES; w++)
			if (w >= wave) rank += wave_count[q][w];
	}
}

// ---- B ----

#define RSZ_BLOCK 256
#define RSZ_OP_MASK 3u
#define RSZ_PER_ELEMENT 4u       // meta bit 2: a flag byte per element
#define RSZ_VEC 8u               // meta bit 3: 16-byte pieces
#define RSZ_MASK_SHIFT 8         // meta bits 8-15: flag_mask
#define RSZ_COL_SHIFT 16         // meta bits 16-26: clamp_col (<= 1024)
static_assert(BSR_RESIZE_CHUNK % (4 * RSZ_BLOCK) == 0, "a chunk is whole 16-byte pieces for every thread");
static_assert(BSR_RESIZE_MAX_WIDTH <= 1024, "clamp_col takes eleven bits of meta");

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct ResizePack {
	const uint32_t* src[BSR_RESIZE_MAX_TENSORS];
	uint32_t* dst[BSR_RESIZE_MAX_TENSORS];
	const uint32_t* append[BSR_RESIZE_MAX_TENSORS];
	const unsigned char* flags[BSR_RESIZE_MAX_TENSORS];
	int width[BSR_RESIZE_MAX_TENSORS];
	uint32_t meta[BSR_RESIZE_MAX_TENSORS];
	uint32_t fill[BSR_RESIZE_MAX_TENSORS];
	float clamp[BSR_RESIZE_MAX_TENSORS];
	int start[BSR_RESIZE_MAX_TENSORS + 1];   // first workgroup of each tensor; start[n] = the grid
};
static_assert(sizeof(ResizePack) + 64 <= 4096, "the descriptors must fit the kernel-argument block");

struct ResizeTensor {   // one tensor's descriptor, in scalar registers
	const uint32_t* src;
	uint32_t* dst;
	const uint32_t* append;
	const unsigned char* flags;
	uint32_t meta, fill;
	float clamp;
	int width;
};

template <int V> struct Piece;
template <> struct Piece<1> { typedef uint32_t type; };
template <> struct Piece<4> { typedef u4 type; };

__device__ __forceinline__ uint32_t piece_get(const u4& p, int j) { return p[j]; }
__device__ __forceinline__ uint32_t piece_get(const uint32_t& p, int) { return p; }
__device__ __forceinline__ void piece_set(u4& p, int j, uint32_t v) { p[j] = v; }
__device__ __forceinline__ void piece_set(uint32_t& p, int, uint32_t v) { p = v; }

// `count` pieces of V elements from piece `base` of the tensor's output on
template <int V>
__device__ __forceinline__ void resize_chunk(const ResizeTensor& T, int base, int count, int N, int n_keep,
                                             const int* __restrict__ src_of)
{
	typedef typename Piece<V>::type P;
	constexpr int PER = BSR_RESIZE_CHUNK / V / RSZ_BLOCK;
	const int wp = T.width / V;                            // pieces of a row
	const int step_rows = RSZ_BLOCK / wp, step_cols = RSZ_BLOCK % wp;
	const uint32_t op = T.meta & RSZ_OP_MASK, mask = (T.meta >> RSZ_MASK_SHIFT) & 0xffu;
	const int clamp_col = (int)((T.meta >> RSZ_COL_SHIFT) & 0x7ffu);
	const bool flagged = op == BSR_RESIZE_ZERO_FLAGGED && T.flags != nullptr;
	int row = (base + (int)threadIdx.x) / wp;
	int col = base + (int)threadIdx.x - row * wp;
	int rows[PER], cols[PER], from[PER];
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const bool valid = (int)threadIdx.x + k * RSZ_BLOCK < count;
		rows[k] = row;
		cols[k] = col;
		int r = -1;
		if (valid && row < n_keep) {
			r = src_of[row];
			if (r < 0 || r >= N) r = -1;
		}
		from[k] = r;
		row += step_rows;
		col += step_cols;
		if (col >= wp) {
			col -= wp;
			row += 1;
		}
	}
	P val[PER];
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		P v = {};
		if ((int)threadIdx.x + k * RSZ_BLOCK < count) {
			if (rows[k] < n_keep) {
				if (from[k] >= 0) {
					const size_t at = (size_t)from[k] * wp + cols[k];
					v = ((const P*)T.src)[at];
					if (flagged) {
						if (T.meta & RSZ_PER_ELEMENT) {
#pragma unroll
							for (int j = 0; j < V; ++j)
								if (T.flags[at * V + j] & mask) piece_set(v, j, 0u);
						} else if (T.flags[from[k]] & mask) {
							v = P{};
						}
					}
				}
			} else if (T.append) {
				v = ((const P*)T.append)[(size_t)(rows[k] - n_keep) * wp + cols[k]];
			} else {
#pragma unroll
				for (int j = 0; j < V; ++j) piece_set(v, j, T.fill);
			}
		}
		val[k] = v;
	}
	P* out = (P*)T.dst + base;
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const int i = (int)threadIdx.x + k * RSZ_BLOCK;
		if (i < count) {
			P v = val[k];
			if (op == BSR_RESIZE_CLAMP_FROM) {
#pragma unroll
				for (int j = 0; j < V; ++j) {
					const float f = __uint_as_float(piece_get(v, j));
					if (cols[k] * V + j >= clamp_col && f > T.clamp) piece_set(v, j, __float_as_uint(T.clamp));
				}
			}
			out[i] = v;
		}
	}
}

__global__ void __launch_bounds__(RSZ_BLOCK) k_rows_resize(const ResizePack a, int n, int N, int n_keep, int A,
                                                           const int* __restrict__ src_of)
{
	const int b = blockIdx.x;
	// the last tensor t with start[t] <= b (adam.hip: k_adam)
	int t = 0, hi = n;
	while (hi - t > 1) {
		const int mid = (t + hi) >> 1;
		if (a.start[mid] <= b) t = mid;
		else hi = mid;
	}
	ResizeTensor T;
	T.src = a.src[t];
	T.dst = a.dst[t];
	T.append = a.append[t];
	T.flags = a.flags[t];
	T.meta = a.meta[t];
	T.fill = a.fill[t];
	T.clamp = a.clamp[t];
	T.width = a.width[t];
	const int total = (n_keep + A) * T.width;                    // < 2^31
	const int base = (b - a.start[t]) * BSR_RESIZE_CHUNK;        // < total
	const int count = min(BSR_RESIZE_CHUNK, total - base);
	if (T.meta & RSZ_VEC) resize_chunk<4>(T, base >> 2, count >> 2, N, n_keep, src_of);   // (width % 4 == 0: whole pieces)
	else resize_chunk<1>(T, base, count, N, n_keep, src_of);
}

static int launch_resize(const char* who, const bsr_resize_tensor* const* batch, int n, int N, int n_keep, int A,
                         const int* src_of, hipStream_t st)
{
	ResizePack a;
	long long blocks = 0;
	for (int k = 0; k < BSR_RESIZE_MAX_TENSORS; ++k) {
		const bsr_resize_tensor* t = batch[k < n ? k : n - 1];   // the unused slots repeat the last tensor: never read
		a.src[k] = (const uint32_t*)t->src;
		a.dst[k] = (uint32_t*)t->dst;
		a.append[k] = A > 0 ? (const uint32_t*)t->append : nullptr;
		a.flags[k] = t->flags;
		a.width[k] = t->width;
		const uintptr_t low = (uintptr_t)t->dst | (n_keep > 0 ? (uintptr_t)t->src : 0) | (A > 0 ? (uintptr_t)t->append : 0);
		const bool vec = t->width % 4 == 0 && (low & 15) == 0;
		a.meta[k] = (uint32_t)t->op | (t->flags_per_element ? RSZ_PER_ELEMENT : 0u) | (vec ? RSZ_VEC : 0u) |
		            ((t->flag_mask & 0xffu) << RSZ_MASK_SHIFT) |
		            (t->op == BSR_RESIZE_CLAMP_FROM ? (uint32_t)t->clamp_col << RSZ_COL_SHIFT : 0u);
		a.fill[k] = t->fill;
		a.clamp[k] = t->clamp;
		a.start[k] = (int)blocks;
		if (k < n) blocks += ((long long)(n_keep + A) * t->width + BSR_RESIZE_CHUNK - 1) / BSR_RESIZE_CHUNK;
	}
	a.start[BSR_RESIZE_MAX_TENSORS] = (int)blocks;   // (64 tensors below 2^31 elements: at most 2^25 workgroups)
	hipLaunchKernelGGL(k_rows_resize, dim3((unsigned)blocks), dim3(RSZ_BLOCK), 0, st, a, n, N, n_keep, A, src_of);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

static size_t count_blocks(long long rows) { return (size_t)((rows + ADJ_SCAN - 1) / ADJ_SCAN); }

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_adjust_decide_scratch_bytes(int N)
{
	if (N <= 0) return 0;
	const size_t blocks_a = count_blocks(N);
	return align_up((2 * blocks_a + count_blocks((long long)N * BSR_ADJUST_MAX_K)) * sizeof(uint32_t), 256);
}

int bsr_adjust_decide(int N, int K, const float* opacity_accum, const float* anchor_demon,
                      const float* offset_gradient_accum, const float* offset_denom, int L, const double* thresholds,
                      double offset_count_min, double anchor_count_min, double min_opacity,
                      unsigned char* offset_flags, unsigned char* anchor_flags, int* src_of, unsigned int* status,
                      void* scratch, void* stream)
{
	const char* who = "bsr_adjust_decide";
	g_err[0] = 0;
	if (N < 0) return fail("%s: N must be >= 0 (got %d)", who, N);
	if (K < 1 || K > BSR_ADJUST_MAX_K) return fail("%s: K must be in [1, %d] (got %d)", who, BSR_ADJUST_MAX_K, K);
	if ((long long)N * K >= 0x80000000LL) return fail("%s: N * K must be below 2^31 (got %d * %d)", who, N, K);
	if (L < 1 || L > BSR_ADJUST_MAX_LEVELS) return fail("%s: L must be in [1, %d] (got %d)", who, BSR_ADJUST_MAX_LEVELS, L);
	if (!thresholds) return fail("%s: NULL thresholds", who);
	DecideScalars s;
	for (int i = 0; i < BSR_ADJUST_MAX_LEVELS; i++) {
		if (i < L && std::isnan(thresholds[i])) return fail("%s: thresholds[%d] is NaN", who, i);
		s.thr[i] = i < L ? (float)thresholds[i] : 0.0f;
	}
	if (std::isnan(offset_count_min)) return fail("%s: offset_count_min is NaN", who);
	if (std::isnan(anchor_count_min)) return fail("%s: anchor_count_min is NaN", who);
	if (std::isnan(min_opacity)) return fail("%s: min_opacity is NaN", who);
	s.L = L;
	s.offset_count_min = (float)offset_count_min;
	s.anchor_count_min = (float)anchor_count_min;
	s.min_opacity = (float)min_opacity;
	if (!status) return fail("%s: NULL status", who);
	if ((uintptr_t)status & 3) return fail("%s: status must be 4-byte aligned", who);
	if (N == 0) return 0;   // nothing to decide: no launch
	if (!opacity_accum || !anchor_demon || !offset_gradient_accum || !offset_denom) return fail("%s: NULL statistic", who);
	if (!offset_flags || !anchor_flags || !src_of) return fail("%s: NULL output", who);
	if (!scratch) return fail("%s: NULL scratch", who);
	if (((uintptr_t)scratch | (uintptr_t)src_of) & 3) return fail("%s: scratch and src_of must be 4-byte aligned", who);
	hipStream_t st = (hipStream_t)stream;
	const int blocks_a = (int)count_blocks(N), blocks_o = (int)count_blocks((long long)N * K);
	uint32_t* keep_count = (uint32_t*)scratch;
	uint32_t* am_count = keep_count + blocks_a;
	uint32_t* om_count = am_count + blocks_a;   // blocks_o <= the BSR_ADJUST_MAX_K blocks an anchor block was sized for
	hipLaunchKernelGGL(k_decide_flags, dim3((unsigned)(blocks_o + blocks_a)), dim3(ADJ_BLOCK), 0, st, N, K, blocks_o,
	                   opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, s, offset_flags, anchor_flags,
	                   keep_count, am_count, om_count);
	hipLaunchKernelGGL(k_decide_plan, dim3((unsigned)blocks_a), dim3(ADJ_BLOCK), 0, st, N, blocks_a,
	                   blocks_o, (const unsigned char*)anchor_flags, (const uint32_t*)keep_count, (const uint32_t*)am_count,
	                   (const uint32_t*)om_count, src_of, (uint32_t*)status);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

int bsr_resize_max_tensors(void)
{
	return BSR_RESIZE_MAX_TENSORS;
}

int bsr_rows_resize(int n_tensors, const bsr_resize_tensor* tensors, int N, int n_keep, int A, const int* src_of, void* stream)
{
	const char* who = "bsr_rows_resize";
	g_err[0] = 0;
	if (n_tensors < 0) return fail("%s: need n_tensors >= 0 (got %d)", who, n_tensors);
	if (n_tensors > 0 && !tensors) return fail("%s: NULL tensor array", who);
	if (N < 0) return fail("%s: N must be >= 0 (got %d)", who, N);
	if (n_keep < 0) return fail("%s: n_keep must be >= 0 (got %d)", who, n_keep);
	if (A < 0) return fail("%s: A must be >= 0 (got %d)", who, A);
	if (n_keep > N) return fail("%s: n_keep must be <= N (got %d > %d)", who, n_keep, N);
	if (n_keep > 0 && n_tensors > 0 && !src_of) return fail("%s: NULL src_of", who);
	if ((uintptr_t)src_of & 3) return fail("%s: src_of must be 4-byte aligned", who);
	const long long rows = (long long)n_keep + A;
	for (int k = 0; k < n_tensors; ++k) {
		const bsr_resize_tensor& t = tensors[k];
		if (t.width < 1 || t.width > BSR_RESIZE_MAX_WIDTH)
			return fail("%s: tensor %d: width must be in [1, %d] (got %d)", who, k, BSR_RESIZE_MAX_WIDTH, t.width);
		if (t.op != BSR_RESIZE_COPY && t.op != BSR_RESIZE_ZERO_FLAGGED && t.op != BSR_RESIZE_CLAMP_FROM)
			return fail("%s: tensor %d: unknown op %d", who, k, t.op);
		if (rows * t.width >= 0x80000000LL)
			return fail("%s: tensor %d: (n_keep + A) * width must be below 2^31 (got %lld * %d)", who, k, rows, t.width);
		if (rows == 0) continue;
		if (!t.dst) return fail("%s: tensor %d: NULL dst", who, k);
		if (n_keep > 0 && !t.src) return fail("%s: tensor %d: NULL src", who, k);
		if (t.op == BSR_RESIZE_ZERO_FLAGGED) {
			if (n_keep > 0 && !t.flags) return fail("%s: tensor %d: NULL flags with BSR_RESIZE_ZERO_FLAGGED", who, k);
			if (t.flag_mask > 0xffu) return fail("%s: tensor %d: flag_mask must be at most 0xff (got 0x%x)", who, k, t.flag_mask);
		}
		if (t.op == BSR_RESIZE_CLAMP_FROM && (t.clamp_col < 0 || t.clamp_col > t.width))
			return fail("%s: tensor %d: clamp_col must be in [0, width] (got %d, width %d)", who, k, t.clamp_col, t.width);
		if (((uintptr_t)t.dst | (uintptr_t)t.src | (uintptr_t)t.append) & 3)
			return fail("%s: tensor %d: src, dst and append must be 4-byte aligned", who, k);
	}
	if (n_tensors == 0 || rows == 0) return 0;
	for (int k = 0; k < n_tensors; ++k) {
		const size_t out = (size_t)rows * tensors[k].width * 4;
		for (int j = 0; j < n_tensors; ++j) {
			const size_t w = (size_t)tensors[j].width * 4;
			if (overlap(tensors[k].dst, out, tensors[j].src, n_keep > 0 ? (size_t)N * w : 0) ||
			    overlap(tensors[k].dst, out, tensors[j].append, (size_t)A * w))
				return fail("%s: tensor %d: dst overlaps a src or an append (of tensor %d)", who, k, j);
		}
	}
	hipStream_t st = (hipStream_t)stream;
	const bsr_resize_tensor* batch[BSR_RESIZE_MAX_TENSORS];
	int n = 0;
	for (int k = 0; k <= n_tensors; ++k) {
		if (k < n_tensors) batch[n++] = &tensors[k];
		if (n == BSR_RESIZE_MAX_TENSORS || (k == n_tensors && n > 0)) {
			if (const int rc = launch_resize(who, batch, n, N, n_keep, A, src_of, st)) return rc;
			n = 0;
		}
	}
	return 0;
}

}  // extern "C"
