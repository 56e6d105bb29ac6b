// The internal launch interface: what api.hip calls and the units that hold the kernels define, declared once.
#pragma once
#include "common.h"

namespace bsr {

// Which second binning pass a forward call runs (binning.hip: binning_plan decides, from sizes alone):
//   RADIX   tile ids beyond 16 bits: the remaining LSD radix passes + k_tile_ranges, then the per-tile sort launches,
//   CHAIN   tile-owned chain k_tile_count -> k_tile_starts -> k_tile_scatter, then the per-tile sort launches,
//   BUCKET  k_bucket_sort<area, tiles per wave>: second pass and sort in one launch (tile_sort.hip).
// area: keys per tile area, BUCKET only (512: two tiles per wave; 1024, 2048: one), else 0.  compact: the elements are
// written in their 8-byte form (common.h: load_elem_m).
struct BinPlan {
	enum Form { RADIX, CHAIN, BUCKET } form;
	int area, compact;
};

// One backward tile walk (host side only: the kernels take these as individual arguments).
struct RenderBwdArgs {
	int gx, gy, W, H;
	const uint2* tile_range;
	const uint32_t* point_list;
	const float4* rec;
	const uint32_t* wg_base;
	const float* bg;
	const float* final_T;
	const uint32_t* n_contrib;
	const float* dL_dpix;
	const float* out_depth;   // the depth-gradient extension: both or neither
	const float* dL_depths;
	int* masks_flag;          // forward's hand-over word (flags[6]; flags[2] = kept instances)
	float4* slab;             // [capacity][9 or 10 floats]
	bool strict;              // BSR_FLAG_EXACT_GRAD: k_render_bwd_strict instead of k_render_bwd_t
	int capacity;             // the R the call was handed
};

void launch_preprocess(const PreArgs& a, bool filter_only, hipStream_t s);
void launch_mark_visible(int P, const float* means3D, const float* vm, uint8_t* present, hipStream_t s);
void launch_visible_filter_views(int P, int V, const float* means3D, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* viewmatrices,
                                 const float* projmatrices, int W, int H, float tan_fovx, float tan_fovy, int* radii,
                                 const int* group_of_view, int n_groups, uint8_t* group_mask, uint32_t* wg_counts,
                                 uint32_t* group_counts, hipStream_t s);
void launch_pack_rows(int R, int P, int n_src, const float* const* src, const int* widths, const int64_t* idx,
                      int idx_stride, float* dst_packed, float* const* dst_each, hipStream_t s);
void launch_scans(int n_wg, uint32_t* wg_kept, uint32_t* wg_area, int* flags, uint32_t* hist1, int* host_counts,
                  hipStream_t s);
BinPlan binning_plan(int P, int T, int capacity, long long kept_hint);
void launch_binning(const BinPlan& plan, int P, int T, int gx, const int* n_ptr, int capacity, const GeomState& geom,
                    BinElem* elems_a, BinElem* elems_b, uint32_t* hist, int hist_blocks_max, uint2* tile_range,
                    uint32_t* big_tiles, int* flags, BinElem** elems_sorted, BinElem** elems_free, hipStream_t s);
void launch_sort_tiles(const BinPlan& plan, int T, int n_bound, const int* n_ptr, int capacity, uint2* tile_range,
                       const uint32_t* big_tiles, const int* flags, const uint32_t* digit_total1, const BinElem* elems,
                       BinElem* elems_free, uint32_t* point_list, int force_int, int small_grids, hipStream_t s);
void launch_render_fwd(int gx, int gy, int n_views, int W, int H, const int* n_ptr, int capacity, const uint2* tile_range,
                       uint32_t* point_list, int* masks_flag,
                       const float4* rec, const float* bg, float* final_T, uint32_t* n_contrib, float* out_color,
                       float* out_depth, bool exact_exp, bool nan_on_overflow, int* pool_ctr, hipStream_t s);
void launch_render_bwd(const RenderBwdArgs& a, hipStream_t s);          // render_bwd.hip: dispatches on a.strict
void launch_render_bwd_strict(const RenderBwdArgs& a, hipStream_t s);   // render_bwd_strict.hip
void launch_preprocess_bwd(const BwdArgs& a, hipStream_t s);

}  // namespace bsr
