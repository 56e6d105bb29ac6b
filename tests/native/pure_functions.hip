// Test-only: the product's PURE functions, compiled from the product's own headers and run on given inputs, so
// that the python restatements of tests/test_box_test_cpu.py, test_tile_pool_cpu.py, test_bin_elem_cpu.py and
// test_scratch_layout_cpu.py are checked
// against the code the kernels execute (an edit to box_may_hit, pooled_tile or the element packing would
// otherwise leave those CPU tests green).  Also the backward walks' cross-lane sum networks (bwd_sums.h) on given
// per-lane inputs, for tests/test_bwd_sums_gpu.py.  Built by tests/native/Makefile into libbsr_pure_functions.so; driven by
// tests/test_round6_gpu.py and tests/test_bwd_sums_gpu.py through ctypes.  Nothing here is part of the product library.
// (The shared workgroup scans of wg_scan.h, the grid-wide fp64 sum of grid_sum.h and the weight-gradient sums of
// mlp_wgrad.{h,hip} have a unit of their own beside this one, shared_pieces.hip -> libbsr_shared_pieces.so, built with the
// product's own flags: tests/test_wg_scan_gpu.py, test_grid_sum_gpu.py and test_mlp_wgrad_direct_gpu.py.)
#include "../../bloomscene_amd/csrc/tile_common.h"
#include "../../bloomscene_amd/csrc/bwd_sums.h"
#include "../../bloomscene_amd/csrc/scratch.h"

using namespace bsr;

// out[i] = box_may_hit<EXT, EXTY>(...) with the derived arguments formed exactly as the callers form them
// (tile_common.h: stage_and_compact_s; preprocess.hip: the exact tile cull)
template <int EXT, int EXTY>
__global__ void k_box(int n, const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ a,
                      const float* __restrict__ b, const float* __restrict__ c, const float* __restrict__ cut,
                      const float* __restrict__ bx, const float* __restrict__ by, unsigned char* __restrict__ out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool pd = (a[i] > 0.0f) && (c[i] > 0.0f) && (a[i] * c[i] - b[i] * b[i] > 0.0f);
	const float rb_c = -b[i] / c[i], rb_a = -b[i] / a[i];
	out[i] = box_may_hit<EXT, EXTY>(X[i], Y[i], a[i], b[i], c[i], cut[i], rb_c, rb_a, pd, bx[i], by[i]) ? 1 : 0;
}

// element packing: store_elem_m -> load_elem_m / elem_tile_m / elem_key_m through a scratch buffer of 12 B per element
__global__ void k_elem(int n, int compact, const uint32_t* __restrict__ tile, const uint32_t* __restrict__ id,
                       const uint32_t* __restrict__ depth, BinElem* __restrict__ scratch, uint32_t* __restrict__ o_tile,
                       uint32_t* __restrict__ o_id, uint32_t* __restrict__ o_depth, uint32_t* __restrict__ o_tile_only,
                       unsigned long long* __restrict__ o_key)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	store_elem_m(scratch, (size_t)i, BinElem{tile[i], id[i], depth[i]}, compact);
	__threadfence();
	const BinElem e = load_elem_m(scratch, (size_t)i, compact);
	o_tile[i] = e.x; o_id[i] = e.y; o_depth[i] = e.z;
	o_tile_only[i] = elem_tile_m(scratch, (size_t)i, compact);
	o_key[i] = elem_key_m(scratch, (size_t)i, compact);
}

// the tile walks' workgroup -> tile assignment: every workgroup of a pooled launch records what pooled_tile hands it
__global__ void __launch_bounds__(256) k_pool(int n_tiles, int* pool_ctr, int* __restrict__ tile_of_wg)
{
	__shared__ int s_slot;
	const int t = pooled_tile((int)blockIdx.x, n_tiles, pool_ctr, &s_slot);
	if (threadIdx.x == 0) tile_of_wg[blockIdx.x] = t;
}

// One wave runs one of bwd_sums.h's networks on in[v][lane] (10 x 64 floats).  network 0: wave_sums_masked ->
// out[0][lane] = the value the lane ends with, aux[lane] = calibrate_components' component of the lane,
// aux[64 + lane] = whether the lane stores it.  network 1: row8_sums, 2: row4_sums -> out[v][lane] = register v of the lane.
template <bool TEN>
__global__ void __launch_bounds__(64) k_bwd_sums(int network, const float* __restrict__ in, float* __restrict__ out,
                                                 int* __restrict__ aux)
{
	const int lane = threadIdx.x;
	float x[10];
#pragma unroll
	for (int v = 0; v < 10; v++) x[v] = in[v * 64 + lane];
	if (network == 0) {
		bool stores;
		aux[lane] = calibrate_components<TEN>(lane, stores);
		aux[64 + lane] = stores ? 1 : 0;
		out[lane] = wave_sums_masked<TEN>(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9]);
		return;
	}
	if (network == 1) row8_sums<TEN>(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9]);
	else row4_sums<TEN>(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9]);
#pragma unroll
	for (int v = 0; v < 10; v++) out[v * 64 + lane] = x[v];
}

extern "C" {

// in, out: 10 x 64 floats; aux: 2 x 64 ints (network 0 only)
int pt_bwd_sums(int network, int ten, const float* in, float* out, int* aux, void* stream)
{
	if (network < 0 || network > 2) return 1;
	if (ten) hipLaunchKernelGGL((k_bwd_sums<true>), dim3(1), dim3(64), 0, (hipStream_t)stream, network, in, out, aux);
	else hipLaunchKernelGGL((k_bwd_sums<false>), dim3(1), dim3(64), 0, (hipStream_t)stream, network, in, out, aux);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

int pt_box_may_hit(int ext, int exty, int n, const float* X, const float* Y, const float* a, const float* b, const float* c,
                   const float* cut, const float* bx, const float* by, unsigned char* out, void* stream)
{
	hipStream_t s = (hipStream_t)stream;
	const dim3 g((n + 255) / 256), blk(256);
	if (ext == 15 && exty == 15) hipLaunchKernelGGL((k_box<15, 15>), g, blk, 0, s, n, X, Y, a, b, c, cut, bx, by, out);
	else if (ext == 7 && exty == 7) hipLaunchKernelGGL((k_box<7, 7>), g, blk, 0, s, n, X, Y, a, b, c, cut, bx, by, out);
	else if (ext == 7 && exty == 3) hipLaunchKernelGGL((k_box<7, 3>), g, blk, 0, s, n, X, Y, a, b, c, cut, bx, by, out);
	else return 1;
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

int pt_elem_roundtrip(int n, int compact, const uint32_t* tile, const uint32_t* id, const uint32_t* depth, void* scratch,
                      uint32_t* o_tile, uint32_t* o_id, uint32_t* o_depth, uint32_t* o_tile_only, unsigned long long* o_key,
                      void* stream)
{
	hipLaunchKernelGGL(k_elem, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, compact, tile, id, depth,
	                   (BinElem*)scratch, o_tile, o_id, o_depth, o_tile_only, o_key);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// (host side: no GPU) the bucket of every depth of a segment, as rank_sort computes it
void pt_rank_sort_buckets(int n, const float* z, float zmin, float zmax, int nb, unsigned int* out)
{
	const float scale = rank_sort_scale(zmin, zmax, nb);
	for (int i = 0; i < n; i++) out[i] = rank_sort_bucket(z[i], zmin, scale, nb);
}
// (host side: no GPU) scratch.h: the three totals, then the offset of every section from a 256-byte aligned base, in
// the order of the struct members (9 of GeomState, 5 of BinState, 5 of ImgState), then the two slab constants
void pt_scratch_layout(size_t P, size_t R, int with_slab, size_t N, size_t T, size_t* out)
{
	char* const base = (char*)(size_t)(1 << 20);
	const GeomState g = GeomState::carve(base, P);
	const BinState b = BinState::carve(base, R, with_slab != 0);
	const ImgState i = ImgState::carve(base, N, T);
	const void* const sections[] = {g.rec, g.inst_offset, g.wg_kept, g.wg_area, g.hist1, g.kept_mask, g.rect, g.clamped, g.depth,
	                                b.point_list, b.elems_a, b.elems_b, b.slab, b.hist,
	                                i.final_T, i.n_contrib, i.tile_range, i.flags, i.big_tiles};
	*out++ = GeomState::bytes(P);
	*out++ = BinState::bytes(R, with_slab != 0);
	*out++ = ImgState::bytes(N, T);
	for (const void* p : sections) *out++ = (size_t)((const char*)p - base);
	*out++ = BSR_SLAB_ROW_BYTES;
	*out++ = BSR_SLAB_TAIL_BYTES;
}
int pt_pooled_grid(int n_tiles) { return pooled_grid(n_tiles); }
int pt_pool_tiles_per_band(int n_tiles) { return pool_tiles_per_band(n_tiles); }

// tile_of_wg: pt_pooled_grid(n_tiles) ints; pool_ctr: one zeroed int
int pt_pooled_tiles(int n_tiles, int* pool_ctr, int* tile_of_wg, void* stream)
{
	hipLaunchKernelGGL(k_pool, dim3(pooled_grid(n_tiles)), dim3(256), 0, (hipStream_t)stream, n_tiles, pool_ctr, tile_of_wg);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
