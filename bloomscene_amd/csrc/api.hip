// C ABI (include/bloomscene_rast.h) and host orchestration of the gfx950 rasterizer: every entry point checks its
// arguments, carves the caller's scratch (scratch.h) and launches its stages (launch.h).  The error string and the
// per-thread host state live in host_state.hip, the stage profiler in profiler.hip.
//
// Stage order of one forward call (cf. the reference's CudaRasterizer::Rasterizer::forward,
// cuda_rasterizer/rasterizer_impl.cu:198-339):
//   k_preprocess (project, cull, SH, exact tile cull, Gaussian-major instance numbering)
//   -> k_scans (workgroup bases, totals, pass-1 histogram rows) -> 16-byte D2H read (kept, num_rendered), overlapped with:
//   binning alloc (sized from the previous call) -> k_emit_scatter (= first radix pass) -> k_tile_count ->
//   k_tile_starts -> k_tile_scatter (tile ids of up to 16 bits; else the remaining radix passes -> k_tile_ranges)
//   -> k_sort_tiles_* (per-tile LDS sort) -> k_render_fwd.  No float atomics anywhere.
// Backward (rasterizer_impl.cu:403-504): k_render_bwd_t or k_render_bwd_strict (per-instance partial sums to a Gaussian-major
// slab, no atomics) -> k_preprocess_bwd (adds each Gaussian's adjacent rows, then the chain).
#include "../../include/bloomscene_rast.h"
#include "common.h"
#include "errors.h"
#include "host_state.h"
#include "launch.h"
#include "profiler.h"
#include "scratch.h"

#include <cstring>

using namespace bsr;

// (BSR_FLAG_EXACT_GRAD concerns the backward alone and the others the forward alone: each accepts and ignores the
// other's, so that a caller can hand one word to both)
static constexpr unsigned BSR_KNOWN_FLAGS = BSR_FLAG_EXACT_EXP | BSR_FLAG_EXACT_GRAD | BSR_FLAG_NO_READBACK | BSR_FLAG_TEST_MASK;

static bool is_capturing(hipStream_t s)
{
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
	return cs != hipStreamCaptureStatusNone;
}

static int check_common(int P, int width, int height, const float* means3D, const float* scales, const float* rotations,
                        const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix)
{
	if (P < 0 || width <= 0 || height <= 0) return fail("invalid sizes: P=%d width=%d height=%d", P, width, height);
	if ((width + BSR_TILE - 1) / BSR_TILE > 65535 || (height + BSR_TILE - 1) / BSR_TILE > 65535)
		return fail("image too large for 16-bit tile coordinates");
	if (P > 0 && !means3D) return fail("means3D is null");
	if (!viewmatrix || !projmatrix) return fail("viewmatrix/projmatrix is null");
	const bool has_sr = scales != nullptr && rotations != nullptr;
	const bool has_any_sr = scales != nullptr || rotations != nullptr;
	if (P > 0 && ((!has_sr && !cov3D_precomp) || (has_any_sr && cov3D_precomp)))
		return fail("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
	return 0;
}

// What the forward checks of its inputs once P > 0 (P == 0 needs none of them).
static int check_forward_args(bsr_alloc_fn geometryBuffer, bsr_alloc_fn binningBuffer, bsr_alloc_fn imageBuffer, int P,
                              int D, int M, const float* background, int width, int height, const float* means3D,
                              const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                              const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* cam_pos, const float* out_color,
                              const float* out_depth)
{
	if (check_common(P, width, height, means3D, scales, rotations, cov3D_precomp, viewmatrix, projmatrix)) return 1;
	if (!geometryBuffer || !binningBuffer || !imageBuffer) return fail("scratch allocation callback is null");
	if (!out_color || !out_depth || !background) return fail("out_color/out_depth/background is null");
	if (!opacities) return fail("opacities is null");
	if ((shs == nullptr) == (colors_precomp == nullptr))
		return fail("Please provide excatly one of either SHs or precomputed colors!");
	if (shs && (!cam_pos || M <= 0)) return fail("SH colours need cam_pos and M > 0");
	if (shs && D >= 0 && (D + 1) * (D + 1) > M && D <= 3)
		return fail("sh_degree %d needs %d coefficients per Gaussian, shs holds %d", D, (D + 1) * (D + 1), M);
	return 0;
}

// One forward call past its checks: what the stages behind k_scans take.
struct ForwardCall {
	hipStream_t s;
	unsigned flags;
	int debug;
	bool no_readback;
	int V, P, width, height, gx, gy, T, n_wg;
	size_t P_rows;
	GeomState geom;
	ImgState img;
	bsr_alloc_fn binningBuffer;
	void* binning_user;
	const float* background;
	float *out_color, *out_depth;
	size_t cap;   // what the binning scratch was last carved for
};

// bins, sorts and renders with scratch sized for `capacity` instances; every kernel takes the real count
// from device memory and returns at once if it exceeds the capacity
static int run_tail(ForwardCall& c, size_t capacity, bool rerun, long long kept_hint)
{
	hipStream_t s = c.s;
	const unsigned flags = c.flags;
	const int V = c.V, T = c.T, debug = c.debug;
	const GeomState& geom = c.geom;
	const ImgState& img = c.img;
	char* bin_p = c.binningBuffer(c.binning_user, BinState::bytes(capacity, V == 1));
	if (!bin_p) return fail("scratch allocation callback returned null");
	const BinState bin = BinState::carve(bin_p, capacity, V == 1);
	c.cap = capacity;
	if (rerun) {
		// A first tail that was NOT skipped (kept <= its capacity, but the backward's carve would not fit) has already
		// filed its long tiles: flags[1], [4], [5] count the work lists of the wide sort classes and are zeroed only by
		// k_scans.  Counting again on top of them would list every long tile twice (two workgroups sorting one tile
		// through the same global scratch) and could spill one class's list into the next.
		HIP_TRY(hipMemsetAsync(img.flags + 1, 0, sizeof(int), s));
		HIP_TRY(hipMemsetAsync(img.flags + 4, 0, 2 * sizeof(int), s));
	}
	const int* n_ptr = img.flags + 2;
	const BinPlan plan = binning_plan((int)c.P_rows, T, (int)capacity, kept_hint);
	BinElem* elems_sorted = nullptr;
	BinElem* elems_free = nullptr;
	{
		StageTimer t("binning", s);
		launch_binning(plan, (int)c.P_rows, T, c.gx, n_ptr, (int)capacity, geom, bin.elems_a, bin.elems_b, bin.hist, BSR_HIST_BLOCKS_MAX,
		               img.tile_range, img.big_tiles, img.flags, &elems_sorted, &elems_free, s);
	}
	STAGE_CHECK("binning", debug, s);
	{
		StageTimer t("sort_tiles", s);
		// (the 256 digit totals of pass 1 lie behind the rows of hist1)
		const uint32_t* digit_total1 = geom.hist1 + BSR_RADIX_BINS_ * hist1_columns((size_t)c.n_wg);
		launch_sort_tiles(plan, T, (int)capacity, n_ptr, (int)capacity, img.tile_range, img.big_tiles, img.flags,
		                  digit_total1, elems_sorted, elems_free, bin.point_list,
		                  ((flags & BSR_FLAG_TEST_SORT_INT) ? 1 : 0) | ((flags & BSR_FLAG_TEST_SORT_NETWORK) ? 2 : 0),
		                  (flags & BSR_FLAG_TEST_SMALL_GRIDS) != 0, s);
	}
	STAGE_CHECK("sort_tiles", debug, s);
	{
		StageTimer t("render_fwd", s);
		// one view of at most 2^24 Gaussians: the forward's split-list staging hands its per-half box tests to the
		// backward in the top byte of the point_list words (flags[6] says whether it did)
		int* const masks_flag = (V == 1 && c.P <= (1 << 24) && !(flags & BSR_FLAG_TEST_NO_HALF_MASKS)) ? img.flags + 6 : nullptr;
		launch_render_fwd(c.gx, c.gy, V, c.width, c.height, n_ptr, (int)capacity, img.tile_range, bin.point_list, masks_flag, geom.rec,
		                  c.background, V > 1 ? nullptr : img.final_T, V > 1 ? nullptr : img.n_contrib, c.out_color, c.out_depth,
		                  (flags & BSR_FLAG_EXACT_EXP) != 0, c.no_readback, img.flags + BSR_POOL_FWD, s);
	}
	return 0;
}

// One or several views of the same Gaussians.  V = 1 is bsr_forward_ex (scratch layouts as the backward expects them);
// V > 1 stacks the views into one virtual image of V * gy tile rows (see PreArgs::n_views) so that every kernel
// after k_preprocess runs unchanged over V * T tiles -- the sparse views of a camera sweep are launch/latency
// bound one by one.
static int forward_impl(int V, bsr_alloc_fn geometryBuffer, void* geometry_user, bsr_alloc_fn binningBuffer,
                        void* binning_user, bsr_alloc_fn imageBuffer, void* image_user, int P, int D, int M,
                        const float* background, int width,
                int height, const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth, int* radii,
                int debug, void* stream, int* num_rendered, unsigned flags)
{
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (flags & ~BSR_KNOWN_FLAGS) {
		if (num_rendered) *num_rendered = 0;
		return fail("forward: unknown flag bits 0x%x", flags & ~BSR_KNOWN_FLAGS);
	}
	const bool no_readback = (flags & BSR_FLAG_NO_READBACK) != 0;
	const long long given_capacity = (no_readback && num_rendered) ? (long long)*num_rendered : 0;
	if (num_rendered) *num_rendered = 0;
	if (no_readback) {
		if (V != 1) return fail("BSR_FLAG_NO_READBACK is for single-view calls");
		if (prefiltered) return fail("BSR_FLAG_NO_READBACK cannot be combined with prefiltered (its violation flag is part of the read-back)");
		if (!num_rendered || given_capacity <= 0)
			return fail("BSR_FLAG_NO_READBACK: *num_rendered must hold the capacity (tile instances, > 0) on entry");
	}
	{   // the deferred status of this thread's previous no-readback forward comes first
		SyncCache* sc0 = sync_cache();
		if (!sc0) return 1;
		// the check is a blocking host wait on an event: inside a stream capture that would invalidate the capture
		// (or hang, depending on the capture mode) -- say so instead
		if (sc0->pending && is_capturing(s))
			return fail("forward during stream capture while the overflow check of this thread's previous BSR_FLAG_NO_READBACK "
			            "forward is pending: call bsr_check_deferred() before hipStreamBeginCapture");
		if (check_deferred(sc0)) return 1;
	}
	if (no_readback) *num_rendered = (int)given_capacity;   // what the backward must be handed as R (same carve)
	if (P == 0) {   // reference rasterize_points.cu:68-82: zero images, no scratch, num_rendered = 0
		if (width <= 0 || height <= 0 || !out_color || !out_depth) return fail("invalid image outputs");
		HIP_TRY(hipMemsetAsync(out_color, 0, (size_t)V * 3 * width * height * sizeof(float), s));
		HIP_TRY(hipMemsetAsync(out_depth, 0, (size_t)V * width * height * sizeof(float), s));
		return 0;
	}
	if (check_forward_args(geometryBuffer, binningBuffer, imageBuffer, P, D, M, background, width, height, means3D, shs,
	                       colors_precomp, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
	                       out_color, out_depth))
		return 1;
	const int gx = (width + BSR_TILE - 1) / BSR_TILE, gy = (height + BSR_TILE - 1) / BSR_TILE;
	if ((long long)V * gy > 65535 || (long long)V * gx * gy > 0x3fffffff) return fail("too many views for one call");
	const int T = gx * gy * V;   // tiles of the stacked virtual image
	const size_t N = (size_t)width * height * (size_t)V;
	const int n_wg = ((P + 255) / 256) * V;
	// geometry rows: P for one view (what the backward carves), V * P_pad virtual ids for several
	const size_t P_rows = V == 1 ? (size_t)P : (size_t)n_wg * 256;
	if (P_rows > 0x7fffffffu) return fail("too many (view, Gaussian) pairs for one call");

	char* geom_p = geometryBuffer(geometry_user, GeomState::bytes(P_rows));
	char* img_p = imageBuffer(image_user, ImgState::bytes(N, (size_t)T));
	if (!geom_p || !img_p) return fail("scratch allocation callback returned null");
	ForwardCall c = {s, flags, debug, no_readback, V, P, width, height, gx, gy, T, n_wg, P_rows,
	                 GeomState::carve(geom_p, P_rows), ImgState::carve(img_p, N, (size_t)T),
	                 binningBuffer, binning_user, background, out_color, out_depth, 0};
	const GeomState& geom = c.geom;
	const ImgState& img = c.img;

	// flags[1..7] are initialised by k_scans (which precedes every kernel that counts into or reads them); flags[0] is
	// written by k_preprocess itself, and only for prefiltered calls, so only those pay a memset launch
	if (prefiltered) HIP_TRY(hipMemsetAsync(img.flags, 0, sizeof(int), s));

	{
		PreArgs a;
		memset(&a, 0, sizeof(a));
		a.P = P; a.D = D; a.M = M;
		a.means3D = means3D; a.scales = scales; a.scale_modifier = scale_modifier; a.rotations = rotations;
		a.opacities = opacities; a.shs = shs; a.cov3D_precomp = cov3D_precomp; a.colors_precomp = colors_precomp;
		a.viewmatrix = viewmatrix; a.projmatrix = projmatrix; a.cam_pos = cam_pos;
		a.W = width; a.H = height; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
		a.focal_y = height / (2.0f * tan_fovy);   // reference rasterizer_impl.cu:223-224
		a.focal_x = width / (2.0f * tan_fovx);
		a.gx = gx; a.gy = gy; a.prefiltered = prefiltered; a.radii = radii; a.geom = geom;
		a.flags = img.flags;
		a.n_views = V;
		if (V > 1)   // sparse views: k_preprocess then writes only the non-zero bins of its pass-1 histogram
			HIP_TRY(hipMemsetAsync(geom.hist1, 0, BSR_RADIX_BINS_ * hist1_columns((size_t)n_wg) * sizeof(uint32_t), s));
		{
			StageTimer t("preprocess", s);
			launch_preprocess(a, false, s);
		}
		STAGE_CHECK("preprocess", debug, s);
	}
	SyncCache* sc = sync_cache();
	if (!sc) return 1;
	// k_scans writes the four counters straight into this thread's pinned, device-mapped landing buffer (no copy on the
	// stream) -- unless the stream is capturing: a graph must not carry a pointer into a host thread's buffer, and an
	// event recorded into a graph cannot be waited for on the host anyway
	const bool capturing = no_readback && is_capturing(s);
	{
		StageTimer t("scan_wg", s);
		launch_scans(n_wg, geom.wg_kept, geom.wg_area, img.flags, geom.hist1, capturing ? nullptr : sc->pinned_dev, s);
	}
	STAGE_CHECK("scan_wg", debug, s);

	const CallShape shape{P, width, height, V};
	if (no_readback) {
		// The caller's capacity sizes the scratch; nothing is waited for.  The counters still travel to the pinned buffer
		// (checked by this thread's next forward / bsr_check_deferred) unless the stream is capturing: an event recorded
		// into a graph cannot be waited for on the host.
		if (!capturing) {
			HIP_TRY(hipEventRecord(sc->deferred, s));   // (behind k_scans, which wrote the counters to the pinned buffer)
			sc->pending = true;
			sc->pending_capacity = (size_t)given_capacity;
			sc->pending_shape = shape;
		}
		// the binning plan: from the kept instances of this thread's last CHECKED no-readback forward of the same shape (its
		// counters were read when this call began), else from the capacity alone -- every plan is correct for every input
		if (run_tail(c, (size_t)given_capacity, false, sc->nr_shape == shape ? (long long)sc->nr_kept : 0)) return 1;
		STAGE_CHECK("render_fwd", debug, s);
		return 0;
	}
	// flags[2] = instances kept after the exact tile cull, flags[3] = the reference's num_rendered
	// (sum of rect areas, rasterizer_impl.cu:278-282), which sizes the binning scratch -> host: the one
	// blocking read of the forward pass (the reference has the same one, rasterizer_impl.cu:282).
	//
	// The read is overlapped with the REST of the forward: binning, tile sort and render take the instance
	// count from device memory, so when the previous call on this thread had the same (P, width, height)
	// the scratch is sized from its num_rendered (+25 %, decaying slowly after a large view) BEFORE the
	// read, all remaining kernels are enqueued behind the copy, and the host only waits for the copy's
	// event (to return num_rendered).  If the guess was too small those kernels returned without touching
	// anything and the tail is simply run again with the exact size.
	const bool guess = sc->can_guess(shape);
	HIP_TRY(hipEventRecord(sc->copied, s));   // behind k_scans: the counters are in the pinned buffer when it completes
	if (guess && run_tail(c, sc->guessed_capacity(), false, (long long)sc->last_kept)) return 1;   // the whole rest of the forward is in flight before the host waits
	HIP_TRY(hipEventSynchronize(sc->copied));
	const int h_flag = prefiltered ? sc->pinned[0] : 0;
	const uint32_t h_kept = (uint32_t)sc->pinned[2], h_R = (uint32_t)sc->pinned[3];
	if (h_flag) return fail("Point is filtered although prefiltered is set. This shouldn't happen!");
	if (h_R > 0x7fffffffu) return fail("too many tile instances (%u)", h_R);
	const int R = (int)h_R;
	if (num_rendered) *num_rendered = R;
	sc->remember(shape, h_R, h_kept);
	if (!guess || (size_t)h_kept > c.cap || (V == 1 && !backward_fits(c.cap, (size_t)R, (size_t)h_kept))) {
		// first call of this shape, more kept instances than the guessed scratch holds (the kernels of the first
		// attempt then returned without touching anything), or a buffer the backward's carve would overrun
		if (run_tail(c, (size_t)R, guess, (long long)h_kept)) return 1;
	}
	STAGE_CHECK("render_fwd", debug, s);
	return 0;
}

extern "C" {

int bsr_version(void) { return BSR_VERSION; }

size_t bsr_geometry_bytes(int P) { return GeomState::bytes((size_t)(P > 0 ? P : 0)); }
size_t bsr_binning_bytes(int R) { return BinState::bytes((size_t)(R > 0 ? R : 0), true); }
size_t bsr_transmittance_offset(const void* image_buffer)
{
	return (size_t)((const char*)ImgState::carve((char*)image_buffer, 0, 0).final_T - (const char*)image_buffer);
}
size_t bsr_image_bytes(int W, int H)
{
	const size_t gx = (W + BSR_TILE - 1) / BSR_TILE, gy = (H + BSR_TILE - 1) / BSR_TILE;
	return ImgState::bytes((size_t)W * H, gx * gy);
}

int bsr_read_counts(const char* image_buffer, int width, int height, void* stream, int* kept, int* num_rendered)
{
	g_err[0] = 0;
	if (!image_buffer || width <= 0 || height <= 0) return fail("bsr_read_counts: invalid image buffer / size");
	const size_t gx = (width + BSR_TILE - 1) / BSR_TILE, gy = (height + BSR_TILE - 1) / BSR_TILE;
	ImgState img = ImgState::carve(const_cast<char*>(image_buffer), (size_t)width * height, gx * gy);
	uint32_t k = 0, r = 0;
	if (read_u32_blocking((const uint32_t*)(img.flags + 2), &k, (hipStream_t)stream)) return 1;
	if (read_u32_blocking((const uint32_t*)(img.flags + 3), &r, (hipStream_t)stream)) return 1;
	if (kept) *kept = (int)k;
	if (num_rendered) *num_rendered = (int)r;
	return 0;
}

int bsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream)
{
	(void)projmatrix;
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (P <= 0) return 0;
	if (!means3D || !viewmatrix || !present) return fail("bsr_mark_visible: null pointer");
	{
		StageTimer t("mark_visible", s);
		launch_mark_visible(P, means3D, viewmatrix, present, s);
	}
	STAGE_CHECK("mark_visible", 0, s);
	return 0;
}

int bsr_visible_filter(int P, int M, int width, int height, const float* means3D, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                       int prefiltered, int* radii, int debug, void* stream)
{
	(void)M;
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (check_common(P, width, height, means3D, scales, rotations, cov3D_precomp, viewmatrix, projmatrix)) return 1;
	if (P == 0) return 0;
	if (!radii) return fail("radii is null");
	// prefiltered: the kernel reports a culled point through ONE word of the calling thread's pinned HOST buffer (mapped
	// into the device's address space): no device allocation, nothing to free on an error path
	int* d_flag = nullptr;
	SyncCache* sc = nullptr;
	if (prefiltered) {
		sc = sync_cache();
		if (!sc) return 1;
		sc->pinned[5] = 0;
		d_flag = sc->pinned_dev + 5;
	}
	PreArgs a;
	memset(&a, 0, sizeof(a));
	a.P = P; a.D = 0; a.M = 0;
	a.means3D = means3D; a.scales = scales; a.scale_modifier = scale_modifier; a.rotations = rotations;
	a.cov3D_precomp = cov3D_precomp; a.viewmatrix = viewmatrix; a.projmatrix = projmatrix;
	a.W = width; a.H = height; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
	a.focal_y = height / (2.0f * tan_fovy);
	a.focal_x = width / (2.0f * tan_fovx);
	a.gx = (width + BSR_TILE - 1) / BSR_TILE; a.gy = (height + BSR_TILE - 1) / BSR_TILE;
	a.prefiltered = prefiltered; a.radii = radii; a.flags = d_flag;
	{
		StageTimer t("visible_filter", s);
		launch_preprocess(a, true, s);
	}
	STAGE_CHECK("visible_filter", debug, s);
	if (prefiltered) {
		HIP_TRY(hipStreamSynchronize(s));
		if (sc->pinned[5]) return fail("Point is filtered although prefiltered is set. This shouldn't happen!");
	}
	return 0;
}

int bsr_visible_filter_views(int P, int n_views, int width, int height, const float* means3D, const float* scales,
                             float scale_modifier, const float* rotations, const float* cov3D_precomp,
                             const float* viewmatrices, const float* projmatrices, float tan_fovx, float tan_fovy,
                             int* radii, int debug, void* stream)
{
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (n_views < 0) return fail("n_views must be >= 0");
	if (check_common(P, width, height, means3D, scales, rotations, cov3D_precomp, viewmatrices, projmatrices)) return 1;
	if (P == 0 || n_views == 0) return 0;
	if (!radii) return fail("radii is null");
	{
		StageTimer t("visible_filter_views", s);
		launch_visible_filter_views(P, n_views, means3D, scales, scale_modifier, rotations, cov3D_precomp, viewmatrices,
		                            projmatrices, width, height, tan_fovx, tan_fovy, radii, nullptr, 0, nullptr,
		                            nullptr, nullptr, s);
	}
	STAGE_CHECK("visible_filter_views", debug, s);
	return 0;
}

size_t bsr_visible_groups_scratch_bytes(int P, int n_groups)
{
	if (P <= 0 || n_groups <= 0) return 0;
	return sizeof(uint32_t) * (size_t)n_groups * (((size_t)P + 255) / 256);
}

int bsr_visible_filter_groups(int P, int n_views, int n_groups, int width, int height, const float* means3D,
                              const float* scales, float scale_modifier, const float* rotations,
                              const float* cov3D_precomp, const float* viewmatrices, const float* projmatrices,
                              float tan_fovx, float tan_fovy, const int* group_of_view, uint8_t* group_mask,
                              uint32_t* group_counts, void* count_scratch, int debug, void* stream)
{
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (n_views < 0 || n_groups < 0 || n_groups > 64) return fail("bsr_visible_filter_groups: need 0 <= n_groups <= 64");
	if (check_common(P, width, height, means3D, scales, rotations, cov3D_precomp, viewmatrices, projmatrices)) return 1;
	if (P == 0 || n_groups == 0) {   // (P == 0: group_mask has no elements; n_groups == 0: no rows)
		if (group_counts && n_groups > 0) HIP_TRY(hipMemsetAsync(group_counts, 0, sizeof(uint32_t) * (size_t)n_groups, s));
		return 0;
	}
	if (!group_mask || (n_views > 0 && !group_of_view)) return fail("bsr_visible_filter_groups: NULL buffer");
	if (group_counts && !count_scratch)
		return fail("bsr_visible_filter_groups: group_counts needs count_scratch (bsr_visible_groups_scratch_bytes)");
	{
		StageTimer t("visible_filter_groups", s);
		// per-workgroup partial counts: the caller's scratch, like every other byte of device memory this library uses
		uint32_t* wg_counts = group_counts ? (uint32_t*)count_scratch : nullptr;
		launch_visible_filter_views(P, n_views, means3D, scales, scale_modifier, rotations, cov3D_precomp, viewmatrices,
		                            projmatrices, width, height, tan_fovx, tan_fovy, nullptr, group_of_view, n_groups,
		                            group_mask, wg_counts, group_counts, s);
	}
	STAGE_CHECK("visible_filter_groups", debug, s);
	return 0;
}

static int gather_impl(const char* who, int R, int P, int n_src, const float* const* src, const int* widths,
                       const int64_t* idx, int idx_stride, float* dst_packed, float* const* dst_each, int debug,
                       void* stream)
{
	g_err[0] = 0;
	hipStream_t s = (hipStream_t)stream;
	if (R < 0 || P < 0 || n_src < 1 || n_src > BSR_PACK_MAX_SRC) return fail("%s: need R >= 0, P >= 0 and 1 <= n_src <= 8", who);
	if (!src || !widths) return fail("%s: NULL table", who);
	int row = 0;
	for (int k = 0; k < n_src; k++) {
		if (widths[k] < 1 || !src[k]) return fail("%s: every source needs a pointer and a width >= 1", who);
		row += widths[k];
	}
	if (row > 4096) return fail("%s: more than 4096 floats per row", who);
	if (R == 0) return 0;
	if (!idx || idx_stride < 1 || (!dst_packed && !dst_each)) return fail("%s: NULL buffer", who);
	if (!dst_packed)
		for (int k = 0; k < n_src; k++)
			if (!dst_each[k]) return fail("%s: NULL destination", who);
	{
		StageTimer t(who, s);
		launch_pack_rows(R, P, n_src, src, widths, idx, idx_stride, dst_packed, dst_each, s);
	}
	STAGE_CHECK(who, debug, s);
	return 0;
}

int bsr_pack_rows(int R, int P, int n_src, const float* const* src, const int* widths, const int64_t* idx, int idx_stride,
                  float* dst, int debug, void* stream)
{
	return gather_impl("pack_rows", R, P, n_src, src, widths, idx, idx_stride, dst, nullptr, debug, stream);
}

int bsr_gather_rows(int R, int P, int n_src, const float* const* src, const int* widths, const int64_t* idx,
                    int idx_stride, float* const* dst, int debug, void* stream)
{
	return gather_impl("gather_rows", R, P, n_src, src, widths, idx, idx_stride, nullptr, dst, debug, stream);
}

int bsr_forward(bsr_alloc_fn geometryBuffer, void* geometry_user, bsr_alloc_fn binningBuffer, void* binning_user,
                bsr_alloc_fn imageBuffer, void* image_user, int P, int D, int M, const float* background, int width,
                int height, const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth, int* radii,
                int debug, void* stream, int* num_rendered)
{
	return bsr_forward_ex(geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user, P, D, M,
	                      background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
	                      rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered,
	                      out_color, out_depth, radii, debug, stream, num_rendered, 0u);
}

int bsr_forward_ex(bsr_alloc_fn geometryBuffer, void* geometry_user, bsr_alloc_fn binningBuffer, void* binning_user,
                   bsr_alloc_fn imageBuffer, void* image_user, int P, int D, int M, const float* background, int width,
                   int height, const float* means3D, const float* shs, const float* colors_precomp,
                   const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                   const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                   float tan_fovx, float tan_fovy, int prefiltered, float* out_color, float* out_depth, int* radii,
                   int debug, void* stream, int* num_rendered, unsigned flags)
{
	return forward_impl(1, geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user, P, D, M,
	                    background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
	                    rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, prefiltered,
	                    out_color, out_depth, radii, debug, stream, num_rendered, flags);
}

int bsr_forward_views(bsr_alloc_fn geometryBuffer, void* geometry_user, bsr_alloc_fn binningBuffer, void* binning_user,
                      bsr_alloc_fn imageBuffer, void* image_user, int P, int D, int M, int n_views,
                      const float* background, int width, int height, const float* means3D, const float* shs,
                      const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrices,
                      const float* projmatrices, const float* cam_positions, float tan_fovx, float tan_fovy,
                      int prefiltered, float* out_color, float* out_depth, int* radii, int debug, void* stream,
                      int* num_rendered, unsigned flags)
{
	g_err[0] = 0;
	if (num_rendered) *num_rendered = 0;
	if (n_views < 0) return fail("n_views must be >= 0");
	if (n_views == 0) return 0;
	return forward_impl(n_views, geometryBuffer, geometry_user, binningBuffer, binning_user, imageBuffer, image_user, P, D,
	                    M, background, width, height, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
	                    rotations, cov3D_precomp, viewmatrices, projmatrices, cam_positions, tan_fovx, tan_fovy,
	                    prefiltered, out_color, out_depth, radii, debug, stream, num_rendered, flags);
}

// out_depth == nullptr: the reference's backward (dL_depths ignored); otherwise the depth-gradient extension
int bsr_backward_ex(int P, int D, int M, int R, const float* background, int width, int height,
                    const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                    float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                    const float* out_depth, const float* dL_dpix, const float* dL_depths, float* dL_dmean2D,
                    float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                    float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream, unsigned flags)
{
	g_err[0] = 0;
	(void)colors_precomp;
	if (P > 0 && out_depth && !dL_depths)
		return fail("bsr_backward_ex: out_depth selects the depth-gradient extension, which needs dL_depths");
	hipStream_t s = (hipStream_t)stream;
	// (the forward's flags are accepted and ignored, so that a caller can hand one word to both calls)
	if (flags & ~BSR_KNOWN_FLAGS) return fail("backward: unknown flag bits 0x%x", flags & ~BSR_KNOWN_FLAGS);
	if (P == 0) return 0;
	if (check_common(P, width, height, means3D, scales, rotations, cov3D_precomp, viewmatrix, projmatrix)) return 1;
	if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail("scratch buffer is null");
	if (!dL_dpix || !background) return fail("dL_dpix/background is null");
	if (!dL_dmean2D || !dL_dopacity || !dL_dmean3D) return fail("gradient output is null");
	// intermediate results may be declined (NULL) -- unless they are the gradient of an input that was given
	if (!shs && !dL_dcolor) return fail("dL_dcolor is null but colors_precomp is the colour input");
	if (!scales && !dL_dcov3D) return fail("dL_dcov3D is null but cov3D_precomp is the covariance input");
	if (shs && (M <= 0 || !dL_dsh || !campos)) return fail("SH backward needs M > 0, dL_dsh and campos");
	if (shs && (D < 0 || (D + 1) * (D + 1) > M))
		return fail("sh_degree %d needs %d coefficients per Gaussian, shs holds %d", D, (D + 1) * (D + 1), M);
	if (scales && (!dL_dscale || !dL_drot)) return fail("dL_dscale/dL_drot is null");

	const int gx = (width + BSR_TILE - 1) / BSR_TILE, gy = (height + BSR_TILE - 1) / BSR_TILE;
	const int T = gx * gy;
	const size_t N = (size_t)width * height;
	GeomState geom = GeomState::carve(geom_buffer, (size_t)P);
	ImgState img = ImgState::carve(image_buffer, N, (size_t)T);
	BinState bin = BinState::carve(binning_buffer, (size_t)(R > 0 ? R : 0), true);

	// slab[R][9 or 10] f32 (tight rows): per-instance partial sums, Gaussian-major (kept instances only use the first R_kept rows), in the
	// caller's binning buffer over the forward's dead radix ping-pong buffers.  The forward sized the buffer for R or for
	// a guessed capacity it checked against this very carve (scratch.h: backward_fits): point_list[R], then the rows
	// of the kept instances, end inside it.
	float4* slab = bin.slab;

	if (R > 0) {
		{
			StageTimer t("render_bwd", s);
			RenderBwdArgs w;
			w.gx = gx; w.gy = gy; w.W = width; w.H = height;
			w.tile_range = img.tile_range; w.point_list = bin.point_list; w.rec = geom.rec; w.wg_base = geom.wg_kept;
			w.bg = background; w.final_T = img.final_T; w.n_contrib = img.n_contrib; w.dL_dpix = dL_dpix;
			w.out_depth = out_depth; w.dL_depths = out_depth ? dL_depths : nullptr;
			w.masks_flag = img.flags + 6; w.slab = slab;
			w.strict = (flags & BSR_FLAG_EXACT_GRAD) != 0; w.capacity = R;
			launch_render_bwd(w, s);
		}
		STAGE_CHECK("render_bwd", debug, s);
	}
	BwdArgs a;
	memset(&a, 0, sizeof(a));
	a.P = P; a.D = D; a.M = M;
	a.means3D = means3D; a.radii = radii; a.shs = shs; a.scales = scales; a.rotations = rotations;
	a.scale_modifier = scale_modifier; a.cov3D_precomp = cov3D_precomp; a.viewmatrix = viewmatrix;
	a.projmatrix = projmatrix; a.campos = campos; a.tan_fovx = tan_fovx; a.tan_fovy = tan_fovy;
	a.focal_y = height / (2.0f * tan_fovy);
	a.focal_x = width / (2.0f * tan_fovx);
	a.geom = geom;
	a.slab = slab; a.depth_grad = out_depth != nullptr;
	a.kept_ptr = img.flags + 2; a.capacity = R;
	a.dL_dmean2D = dL_dmean2D; a.dL_dconic = dL_dconic; a.dL_dopacity = dL_dopacity; a.dL_dcolor = dL_dcolor;
	a.dL_dmean3D = dL_dmean3D; a.dL_dcov3D = dL_dcov3D; a.dL_dsh = dL_dsh; a.dL_dscale = dL_dscale; a.dL_drot = dL_drot;
	{
		StageTimer t("preprocess_bwd", s);
		launch_preprocess_bwd(a, s);
	}
	STAGE_CHECK("preprocess_bwd", debug, s);
	return 0;
}

int bsr_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                 char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_depths,
                 float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream)
{
	(void)dL_depths;   // accepted and ignored, as in the reference (backward.cu:457-463,539-554)
	return bsr_backward_ex(P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier,
	                       rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer,
	                       binning_buffer, image_buffer, nullptr, dL_dpix, nullptr, dL_dmean2D, dL_dconic, dL_dopacity,
	                       dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream, 0u);
}

int bsr_backward_depth(int P, int D, int M, int R, const float* background, int width, int height,
                       const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                       float scale_modifier, const float* rotations, const float* cov3D_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                       float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                       const float* out_depth, const float* dL_dpix, const float* dL_depths, float* dL_dmean2D,
                       float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                       float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream)
{
	if (P > 0 && (!out_depth || !dL_depths)) return fail("bsr_backward_depth needs out_depth and dL_depths");
	return bsr_backward_ex(P, D, M, R, background, width, height, means3D, shs, colors_precomp, scales, scale_modifier,
	                       rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, geom_buffer,
	                       binning_buffer, image_buffer, out_depth, dL_dpix, dL_depths, dL_dmean2D, dL_dconic, dL_dopacity,
	                       dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream, 0u);
}

}  // extern "C"
