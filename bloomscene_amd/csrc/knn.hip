// Mean squared distance to the three nearest neighbours for gfx950 (include/bloomscene_knn.h): BloomScene's
// `simple_knn._C.distCUDA2`, restated from simple_knn.cu ("SK") as an exact search over a two-level box hierarchy.
//
//   k_knn_bounds    per-workgroup min / max of the finite points (grid-stride, <= 256 partials)
//   k_knn_morton    reduces the partials, writes (30-bit Morton code, index); a non-finite point gets 0xffffffff and
//                   sorts last.  The quantiser clamps and maps NaN to 0 (SK's float -> uint conversion is UB there: a
//                   zero-extent axis, a planar cloud, divides 0 by 0)
//   4 x (k_knn_hist, k_knn_rowscan, k_knn_scatter)   stable LSD radix sort of the (code, index) pairs, 8 bits a pass:
//                   per-tile digit counts, one exclusive scan per digit over the tiles, then a scatter in which each
//                   wave ranks its 64 keys with ballots (no float atomics; integer LDS atomics only count)
//   k_knn_leaves    the points in sorted order (float4) and one box per leaf of 64 sorted points (finite points only)
//   k_knn_groups    one box per group of 64 leaves (4096 sorted points)
//   k_knn_query     one wave per leaf: its 64 queries are Morton neighbours.  First the wave's own leaf (self
//                   excluded), then every group whose box the wave may need, then every leaf of such a group that
//                   some lane needs; a leaf's 64 points are broadcast from the lanes that loaded them (v_readlane) and
//                   every lane tests all of them.  Done as soon as every lane's third best is 0.
//
// WHY THE PRUNING IS EXACT.  A box [lo, hi] is skipped for query p only when bound(p, box) > s2, the lane's current
// third smallest value, with bound = (gx*gx + gy*gy) + gz*gz and, per axis, g = lo - p if p < lo, p - hi if p > hi, else
// 0 -- the operation order of d.  For a point q in the box and p < lo, the exact difference q - p >= lo - p > 0;
// rounding to nearest is monotone, so fl(q - p) >= fl(lo - p) = g >= 0 (and symmetrically |fl(q - p)| = fl(p - q) >=
// fl(p - hi) when p > hi; g = 0 otherwise is trivially <= |dx|).  Squaring a non-negative value and adding
// non-negative values are monotone in every operand, so bound <= d(p, q) for every q in the box: every such d is > s2
// and cannot change the three smallest values (a candidate enters only when it is strictly smaller than s2).  The wave
// level test replaces p by the box [qlo, qhi] of the wave's queries (g = lo - qhi if qhi < lo, ...): by the same
// argument it is <= the per-lane bound of every lane, and it is compared with the largest s2 of the wave.  Overflow
// keeps the order (an infinite bound means an infinite d, which never counts).  Non-finite points are in no box and
// are never candidates; padding slots hold NaN, whose d is NaN and never counts.  So the result does not depend on the
// order, the box sizes or the bounds: it is the header's function of the input.
#include "common.h"
#include "wg_scan.h"
#include "../../include/bloomscene_knn.h"

namespace bsr {

#define BSR_KNN_BLOCK 256
#define BSR_KNN_BOUNDS_BLOCKS 256
#define BSR_KNN_MORTON_BLOCKS 1024
#define BSR_KNN_TILE 4096          // keys per radix-sort workgroup: 4 waves x 16 chunks of 64
#define BSR_KNN_LEAF 64            // sorted points per leaf box = one wave of queries
#define BSR_KNN_GROUP 64           // leaves per group box
#define BSR_KNN_FLT_MAX 3.402823466e+38f
#define BSR_KNN_INF __builtin_inff()

__device__ __forceinline__ bool knn_finite(float x) { return __builtin_fabsf(x) <= BSR_KNN_FLT_MAX; }

__device__ __forceinline__ float wave_minf(float v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
	return v;
}
__device__ __forceinline__ float wave_maxf(float v)
{
#pragma unroll
	for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
	return v;
}

struct KnnBox { float lx, ly, lz, hx, hy, hz; };

// boxes are stored as two float4 (lo, hi); w unused
__device__ __forceinline__ KnnBox load_box(const float4* b, int i)
{
	const float4 lo = b[2 * i], hi = b[2 * i + 1];
	return KnnBox{lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
}

__device__ __forceinline__ float gap_point(float p, float lo, float hi)
{
	return p < lo ? lo - p : (p > hi ? p - hi : 0.0f);
}
__device__ __forceinline__ float gap_range(float plo, float phi, float lo, float hi)
{
	return phi < lo ? lo - phi : (plo > hi ? plo - hi : 0.0f);
}
// lower bound of d(p, q) over the points q of the box (see the argument at the top)
__device__ __forceinline__ float bound_point(float px, float py, float pz, const KnnBox& b)
{
	const float gx = gap_point(px, b.lx, b.hx), gy = gap_point(py, b.ly, b.hy), gz = gap_point(pz, b.lz, b.hz);
	return (gx * gx + gy * gy) + gz * gz;
}
// lower bound of d(p, q) over p in the query box Q and q in the box
__device__ __forceinline__ float bound_range(const KnnBox& Q, const KnnBox& b)
{
	const float gx = gap_range(Q.lx, Q.hx, b.lx, b.hx), gy = gap_range(Q.ly, Q.hy, b.ly, b.hy),
	            gz = gap_range(Q.lz, Q.hz, b.lz, b.hz);
	return (gx * gx + gy * gy) + gz * gz;
}

// ---- bounds and Morton codes ----

__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_bounds(int P, const float* __restrict__ pts,
                                                              float* __restrict__ partials)
{
	__shared__ float s[4][6];
	float v[6] = {BSR_KNN_INF, BSR_KNN_INF, BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF};
	for (int i = blockIdx.x * BSR_KNN_BLOCK + threadIdx.x; i < P; i += gridDim.x * BSR_KNN_BLOCK) {
		const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
		if (knn_finite(x) && knn_finite(y) && knn_finite(z)) {
			v[0] = fminf(v[0], x); v[1] = fminf(v[1], y); v[2] = fminf(v[2], z);
			v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y); v[5] = fmaxf(v[5], z);
		}
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for (int k = 0; k < 3; k++) { v[k] = wave_minf(v[k]); v[k + 3] = wave_maxf(v[k + 3]); }
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < 6; k++) s[wave][k] = v[k];
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		const int k = threadIdx.x;
		float r = s[0][k];
		for (int w = 1; w < 4; w++) r = k < 3 ? fminf(r, s[w][k]) : fmaxf(r, s[w][k]);
		partials[blockIdx.x * 6 + k] = r;
	}
}

// 10 bits -> every third bit (SK:45-52)
__device__ __forceinline__ uint32_t knn_spread(uint32_t x)
{
	x = (x | (x << 16)) & 0x030000FFu;
	x = (x | (x << 8)) & 0x0300F00Fu;
	x = (x | (x << 4)) & 0x030C30C3u;
	x = (x | (x << 2)) & 0x09249249u;
	return x;
}
// clamped to [0, 1023]; NaN (0 / 0 on a zero-extent axis) -> 0.  Halved so that hi - lo cannot overflow.
__device__ __forceinline__ uint32_t knn_quant(float x, float lo, float inv)
{
	float t = (x * 0.5f - lo * 0.5f) * inv;
	t = t > 0.0f ? t : 0.0f;
	t = t < 1023.0f ? t : 1023.0f;
	return (uint32_t)t;
}

__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_morton(int P, const float* __restrict__ pts, int n_partials,
                                                              const float* __restrict__ partials,
                                                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
	__shared__ float s[4][6];
	__shared__ float s_b[6];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	float v[6] = {BSR_KNN_INF, BSR_KNN_INF, BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF};
	if ((int)threadIdx.x < n_partials) {
#pragma unroll
		for (int k = 0; k < 6; k++) v[k] = partials[threadIdx.x * 6 + k];
	}
#pragma unroll
	for (int k = 0; k < 3; k++) { v[k] = wave_minf(v[k]); v[k + 3] = wave_maxf(v[k + 3]); }
	if (lane == 0) {
#pragma unroll
		for (int k = 0; k < 6; k++) s[wave][k] = v[k];
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		const int k = threadIdx.x;
		float r = s[0][k];
		for (int w = 1; w < 4; w++) r = k < 3 ? fminf(r, s[w][k]) : fmaxf(r, s[w][k]);
		s_b[k] = r;
	}
	__syncthreads();
	// (no finite point: lo = inf, hi = -inf -> every code below is for a non-finite point anyway)
	const float lx = s_b[0], ly = s_b[1], lz = s_b[2];
	const float ix = 1023.0f / (s_b[3] * 0.5f - lx * 0.5f), iy = 1023.0f / (s_b[4] * 0.5f - ly * 0.5f),
	            iz = 1023.0f / (s_b[5] * 0.5f - lz * 0.5f);
	for (int i = blockIdx.x * BSR_KNN_BLOCK + threadIdx.x; i < P; i += gridDim.x * BSR_KNN_BLOCK) {
		const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
		uint32_t code = 0xffffffffu;
		if (knn_finite(x) && knn_finite(y) && knn_finite(z))
			code = knn_spread(knn_quant(x, lx, ix)) | (knn_spread(knn_quant(y, ly, iy)) << 1) |
			       (knn_spread(knn_quant(z, lz, iz)) << 2);
		keys[i] = code;
		vals[i] = (uint32_t)i;
	}
}

// ---- stable LSD radix sort of (key, value), 8 bits a pass ----

// hist[digit * n_tiles + tile] = keys of the tile with that digit
__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_hist(int P, const uint32_t* __restrict__ keys, int shift,
                                                            int n_tiles, uint32_t* __restrict__ hist)
{
	__shared__ uint32_t s_cnt[256];
	s_cnt[threadIdx.x] = 0u;
	__syncthreads();
	const size_t base = (size_t)blockIdx.x * BSR_KNN_TILE;
#pragma unroll 4
	for (int k = 0; k < BSR_KNN_TILE / BSR_KNN_BLOCK; k++) {
		const size_t i = base + (size_t)k * BSR_KNN_BLOCK + threadIdx.x;
		if (i < (size_t)P) atomicAdd(&s_cnt[(keys[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// workgroup d: row d of hist -> exclusive prefix over the tiles, in place; the row total -> totals[d]
__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_rowscan(int n_tiles, uint32_t* __restrict__ hist,
                                                               uint32_t* __restrict__ totals)
{
	__shared__ uint32_t s_w[2 * (BSR_KNN_BLOCK / 64)];
	const uint32_t total = wg_exclusive_scan<BSR_KNN_BLOCK / 64, 1>(n_tiles, hist + (size_t)blockIdx.x * n_tiles, s_w, true);
	if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// Tile t: wave w owns keys [t * 4096 + w * 1024, + 1024), 16 chunks of 64 in order.  A key's place = the digit's base
// (digits below it, all tiles) + the digit's prefix over the earlier tiles + the counts of the earlier waves of this
// tile + the earlier chunks of this wave + its rank among the lanes of its chunk with the same digit (ballots).
__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_scatter(int P, const uint32_t* __restrict__ kin,
                                                               const uint32_t* __restrict__ vin,
                                                               uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                               int shift, int n_tiles, const uint32_t* __restrict__ hist,
                                                               const uint32_t* __restrict__ totals)
{
	__shared__ uint32_t s_run[4][256];
	__shared__ uint32_t s_w[4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
	for (int w = 0; w < 4; w++) s_run[w][tid] = 0u;
	uint32_t run = wg_exclusive_sum<4>(totals[tid], s_w) + hist[(size_t)tid * n_tiles + blockIdx.x];   // (its barrier covers the zeroes too)
	const size_t wbase = (size_t)blockIdx.x * BSR_KNN_TILE + (size_t)wave * (BSR_KNN_TILE / 4);
	constexpr int CHUNKS = BSR_KNN_TILE / 4 / 64;
	for (int c = 0; c < CHUNKS; c++) {
		const size_t i = wbase + (size_t)c * 64 + lane;
		if (i < (size_t)P) atomicAdd(&s_run[wave][(kin[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
#pragma unroll
	for (int w = 0; w < 4; w++) {
		const uint32_t n = s_run[w][tid];
		s_run[w][tid] = run;
		run += n;
	}
	__syncthreads();
	const uint64_t below = (1ull << lane) - 1ull;
	for (int c = 0; c < CHUNKS; c++) {
		const size_t i = wbase + (size_t)c * 64 + lane;
		const bool valid = i < (size_t)P;
		const uint32_t key = valid ? kin[i] : 0u, val = valid ? vin[i] : 0u;
		const uint32_t d = (key >> shift) & 255u;
		uint64_t peers = wave_ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const bool bit = (d >> b) & 1u;
			const uint64_t m = wave_ballot(bit);
			peers &= bit ? m : ~m;
		}
		const uint32_t rank = (uint32_t)__popcll(peers & below);
		const uint32_t start = s_run[wave][d];
		if (valid && start + rank < (uint32_t)P) {   // (always true; a guard against a broken count)
			kout[start + rank] = key;
			vout[start + rank] = val;
		}
		__builtin_amdgcn_wave_barrier();
		if (valid && rank == 0u) s_run[wave][d] = start + (uint32_t)__popcll(peers);   // one lane per digit
		__builtin_amdgcn_wave_barrier();
	}
}

// ---- boxes ----

// wave = leaf: spts[pos] = the point at sorted position pos (NaN beyond P), lbox[leaf] = box of its finite points
// (empty: lo = inf, hi = -inf)
__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_leaves(int P, int n_leaves, const float* __restrict__ pts,
                                                              const uint32_t* __restrict__ order,
                                                              float4* __restrict__ spts, float4* __restrict__ lbox)
{
	const int lane = threadIdx.x & 63;
	const int leaf = blockIdx.x * (BSR_KNN_BLOCK / 64) + (threadIdx.x >> 6);
	if (leaf >= n_leaves) return;
	const int pos = leaf * BSR_KNN_LEAF + lane;
	float x = __builtin_nanf(""), y = x, z = x;
	if (pos < P) {
		const size_t j = order[pos];
		if (j < (size_t)P) { x = pts[3 * j]; y = pts[3 * j + 1]; z = pts[3 * j + 2]; }
	}
	spts[pos] = make_float4(x, y, z, 0.0f);
	const bool fin = knn_finite(x) && knn_finite(y) && knn_finite(z);
	const float lx = wave_minf(fin ? x : BSR_KNN_INF), ly = wave_minf(fin ? y : BSR_KNN_INF),
	            lz = wave_minf(fin ? z : BSR_KNN_INF);
	const float hx = wave_maxf(fin ? x : -BSR_KNN_INF), hy = wave_maxf(fin ? y : -BSR_KNN_INF),
	            hz = wave_maxf(fin ? z : -BSR_KNN_INF);
	if (lane == 0) {
		lbox[2 * leaf] = make_float4(lx, ly, lz, 0.0f);
		lbox[2 * leaf + 1] = make_float4(hx, hy, hz, 0.0f);
	}
}

// wave = group of 64 leaves
__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_groups(int n_leaves, int n_groups, const float4* __restrict__ lbox,
                                                              float4* __restrict__ gbox)
{
	const int lane = threadIdx.x & 63;
	const int g = blockIdx.x * (BSR_KNN_BLOCK / 64) + (threadIdx.x >> 6);
	if (g >= n_groups) return;
	const int l = g * BSR_KNN_GROUP + lane;
	KnnBox b{BSR_KNN_INF, BSR_KNN_INF, BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF, -BSR_KNN_INF};
	if (l < n_leaves) b = load_box(lbox, l);
	const float lx = wave_minf(b.lx), ly = wave_minf(b.ly), lz = wave_minf(b.lz);
	const float hx = wave_maxf(b.hx), hy = wave_maxf(b.hy), hz = wave_maxf(b.hz);
	if (lane == 0) {
		gbox[2 * g] = make_float4(lx, ly, lz, 0.0f);
		gbox[2 * g + 1] = make_float4(hx, hy, hz, 0.0f);
	}
}

// ---- the search ----

// s0 <= s1 <= s2 keep the three smallest values seen; a candidate enters only when it is strictly below s2 (SK's
// updateKBest: `knn[j] > dist`), so NaN, and anything >= FLT_MAX while s2 is still FLT_MAX, never enters
__device__ __forceinline__ void knn_insert(float d, float& s0, float& s1, float& s2)
{
	const float n2 = d < s1 ? s1 : (d < s2 ? d : s2);
	const float n1 = d < s0 ? s0 : (d < s1 ? d : s1);
	const float n0 = d < s0 ? d : s0;
	s0 = n0; s1 = n1; s2 = n2;
}

// Every lane tests its query against the 64 points of a leaf; lane k loaded point k (NaN padding never counts).
// SELF: the wave's own leaf, where lane k skips point k (itself).
template <bool SELF>
__device__ __forceinline__ void knn_leaf(const float4* __restrict__ spts, int leaf, int lane, float px, float py,
                                         float pz, float& s0, float& s1, float& s2)
{
	const float4 q = spts[(size_t)leaf * BSR_KNN_LEAF + lane];
	const int qx = __float_as_int(q.x), qy = __float_as_int(q.y), qz = __float_as_int(q.z);
#pragma unroll
	for (int k = 0; k < 64; k++) {
		const float dx = __int_as_float(__builtin_amdgcn_readlane(qx, k)) - px;
		const float dy = __int_as_float(__builtin_amdgcn_readlane(qy, k)) - py;
		const float dz = __int_as_float(__builtin_amdgcn_readlane(qz, k)) - pz;
		float d = (dx * dx + dy * dy) + dz * dz;
		if (SELF) d = k == lane ? BSR_KNN_INF : d;
		knn_insert(d, s0, s1, s2);
	}
}

__global__ void __launch_bounds__(BSR_KNN_BLOCK) k_knn_query(int P, int n_leaves, int n_groups,
                                                             const float4* __restrict__ spts,
                                                             const float4* __restrict__ lbox,
                                                             const float4* __restrict__ gbox,
                                                             const uint32_t* __restrict__ order, float* __restrict__ out)
{
	const int lane = threadIdx.x & 63;
	const int leaf = blockIdx.x * (BSR_KNN_BLOCK / 64) + (threadIdx.x >> 6);
	if (leaf >= n_leaves) return;   // (wave-uniform)
	const int pos = leaf * BSR_KNN_LEAF + lane;
	const float4 me = spts[pos];
	const float px = me.x, py = me.y, pz = me.z;
	const bool active = pos < P && knn_finite(px) && knn_finite(py) && knn_finite(pz);
	float s0 = BSR_KNN_FLT_MAX, s1 = BSR_KNN_FLT_MAX, s2 = BSR_KNN_FLT_MAX;
	knn_leaf<true>(spts, leaf, lane, px, py, pz, s0, s1, s2);
	// the box of the wave's queries; a lane without a query is done (its s2 counts as 0 in the wave's maximum)
	const KnnBox Q{wave_minf(active ? px : BSR_KNN_INF), wave_minf(active ? py : BSR_KNN_INF),
	               wave_minf(active ? pz : BSR_KNN_INF), wave_maxf(active ? px : -BSR_KNN_INF),
	               wave_maxf(active ? py : -BSR_KNN_INF), wave_maxf(active ? pz : -BSR_KNN_INF)};
	float smax = wave_maxf(active ? s2 : 0.0f);
	for (int gb = 0; gb < n_groups && smax > 0.0f; gb += 64) {
		const int gl = gb + lane;
		bool cand = false;
		if (gl < n_groups) cand = !(bound_range(Q, load_box(gbox, gl)) > smax);
		uint64_t gmask = wave_ballot(cand);
		while (gmask && smax > 0.0f) {
			const int g = gb + __builtin_ctzll(gmask);
			gmask &= gmask - 1ull;
			if (!wave_ballot(active && !(bound_point(px, py, pz, load_box(gbox, g)) > s2))) continue;
			const int l0 = g * BSR_KNN_GROUP;
			const int ll = l0 + lane;
			bool lc = false;
			if (ll < n_leaves && ll != leaf) lc = !(bound_range(Q, load_box(lbox, ll)) > smax);
			uint64_t lmask = wave_ballot(lc);
			while (lmask) {
				const int l = l0 + __builtin_ctzll(lmask);
				lmask &= lmask - 1ull;
				if (!wave_ballot(active && !(bound_point(px, py, pz, load_box(lbox, l)) > s2))) continue;
				knn_leaf<false>(spts, l, lane, px, py, pz, s0, s1, s2);
				smax = wave_maxf(active ? s2 : 0.0f);
				if (!(smax > 0.0f)) break;
			}
		}
	}
	if (pos < P) {
		const uint32_t j = order[pos];
		if (j < (uint32_t)P) out[j] = ((s0 + s1) + s2) / 3.0f;
	}
}

// ---- scratch ----

struct KnnScratch {
	uint32_t *keys_a, *keys_b, *vals_a, *vals_b;   // [P] each
	float* partials;                                // [BSR_KNN_BOUNDS_BLOCKS * 6]
	uint32_t* hist;                                 // [256 * n_tiles]
	uint32_t* totals;                               // [256]
	float4* spts;                                   // [n_leaves * 64]
	float4* lbox;                                   // [2 * n_leaves]
	float4* gbox;                                   // [2 * n_groups]
	int n_tiles, n_leaves, n_groups;
	size_t bytes;
};

static KnnScratch carve_knn_scratch(void* base, size_t P)
{
	KnnScratch s;
	const size_t n_tiles = (P + BSR_KNN_TILE - 1) / BSR_KNN_TILE, n_leaves = (P + BSR_KNN_LEAF - 1) / BSR_KNN_LEAF;
	const size_t n_groups = (n_leaves + BSR_KNN_GROUP - 1) / BSR_KNN_GROUP;
	s.n_tiles = (int)n_tiles; s.n_leaves = (int)n_leaves; s.n_groups = (int)n_groups;
	char* p = (char*)base;
	size_t o = 0;
	auto take = [&](size_t bytes) { char* r = p + o; o += align_up(bytes, 256); return r; };
	s.keys_a = (uint32_t*)take(P * 4);
	s.keys_b = (uint32_t*)take(P * 4);
	s.vals_a = (uint32_t*)take(P * 4);
	s.vals_b = (uint32_t*)take(P * 4);
	s.partials = (float*)take(BSR_KNN_BOUNDS_BLOCKS * 6 * 4);
	s.hist = (uint32_t*)take(256 * n_tiles * 4);
	s.totals = (uint32_t*)take(256 * 4);
	s.spts = (float4*)take(n_leaves * BSR_KNN_LEAF * 16);
	s.lbox = (float4*)take(n_leaves * 32);
	s.gbox = (float4*)take(n_groups * 32);
	s.bytes = o;
	return s;
}

}  // namespace bsr

using namespace bsr;

extern "C" {

size_t bsr_knn_scratch_bytes(int P)
{
	if (P < 0) return 0;
	return carve_knn_scratch(nullptr, (size_t)P).bytes;
}

int bsr_knn_mean_dist(int P, const float* points, float* out, void* scratch, void* stream)
{
	const char* who = "bsr_knn_mean_dist";
	if (P < 0 || P > BSR_KNN_MAX_P) return fail("%s: need 0 <= P <= %d (got %d)", who, BSR_KNN_MAX_P, P);
	if (P == 0) return 0;
	if (!points || !out || !scratch) return fail("%s: NULL buffer", who);
	if (((uintptr_t)points | (uintptr_t)out) & 3) return fail("%s: points / out must be 4-byte aligned", who);
	if ((uintptr_t)scratch & 15) return fail("%s: scratch must be 16-byte aligned", who);
	const KnnScratch s = carve_knn_scratch(scratch, (size_t)P);
	hipStream_t st = (hipStream_t)stream;
	const dim3 blk(BSR_KNN_BLOCK);
	int nb = (P + BSR_KNN_BLOCK - 1) / BSR_KNN_BLOCK;
	const int n_partials = nb < BSR_KNN_BOUNDS_BLOCKS ? nb : BSR_KNN_BOUNDS_BLOCKS;
	hipLaunchKernelGGL(k_knn_bounds, dim3(n_partials), blk, 0, st, P, points, s.partials);
	hipLaunchKernelGGL(k_knn_morton, dim3(nb < BSR_KNN_MORTON_BLOCKS ? nb : BSR_KNN_MORTON_BLOCKS), blk, 0, st, P,
	                   points, n_partials, (const float*)s.partials, s.keys_a, s.vals_a);
	uint32_t *ka = s.keys_a, *kb = s.keys_b, *va = s.vals_a, *vb = s.vals_b;
	for (int shift = 0; shift < 32; shift += 8) {
		hipLaunchKernelGGL(k_knn_hist, dim3(s.n_tiles), blk, 0, st, P, (const uint32_t*)ka, shift, s.n_tiles, s.hist);
		hipLaunchKernelGGL(k_knn_rowscan, dim3(256), blk, 0, st, s.n_tiles, s.hist, s.totals);
		hipLaunchKernelGGL(k_knn_scatter, dim3(s.n_tiles), blk, 0, st, P, (const uint32_t*)ka, (const uint32_t*)va, kb,
		                   vb, shift, s.n_tiles, (const uint32_t*)s.hist, (const uint32_t*)s.totals);
		uint32_t* t = ka; ka = kb; kb = t;
		t = va; va = vb; vb = t;
	}
	// (four passes: the sorted order is back in vals_a)
	const unsigned wg_leaves = (unsigned)((s.n_leaves + 3) / 4), wg_groups = (unsigned)((s.n_groups + 3) / 4);
	hipLaunchKernelGGL(k_knn_leaves, dim3(wg_leaves), blk, 0, st, P, s.n_leaves, points, (const uint32_t*)va, s.spts,
	                   s.lbox);
	hipLaunchKernelGGL(k_knn_groups, dim3(wg_groups), blk, 0, st, s.n_leaves, s.n_groups, (const float4*)s.lbox, s.gbox);
	hipLaunchKernelGGL(k_knn_query, dim3(wg_leaves), blk, 0, st, P, s.n_leaves, s.n_groups, (const float4*)s.spts,
	                   (const float4*)s.lbox, (const float4*)s.gbox, (const uint32_t*)va, out);
	if (hipGetLastError() != hipSuccess) return fail("%s: launch failed", who);
	return 0;
}

}  // extern "C"
