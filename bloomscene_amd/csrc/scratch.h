// The private layout of the three caller-owned scratch buffers (common.h: GeomState, BinState, ImgState), each stated
// ONCE: X::layout lists the sections in order; X::bytes (a Carver without a base: it only counts) and X::carve (the
// same walk over the caller's buffer) both come from it.  Host code, included by the ABI unit (api.hip) alone --
// and by tests/native/pure_functions.hip, which checks it against tests/helpers.py::scratch_offsets.
#pragma once
#include "common.h"

namespace bsr {

static constexpr size_t BSR_RADIX_BINS_ = 256;

// Hands out consecutive 256-byte aligned sections.  base == nullptr: only counts.  (X::bytes adds 256 to the count:
// the caller's buffer need not be aligned, X::carve starts at its first 256-byte boundary.)
struct Carver {
	char* base;
	size_t off = 0;
	template <class T> T* take(size_t n)
	{
		T* r = base ? (T*)(base + off) : nullptr;
		off += align_up(n * sizeof(T), 256);
		return r;
	}
};

// Columns of the digit-major pass-1 histogram (common.h: hist1_column) for n_wg preprocess workgroups.
static inline size_t hist1_columns(size_t n_wg) { return (n_wg + 7) / 8 * 8; }

inline GeomState GeomState::layout(Carver& c, size_t P)
{
	const size_t n_wg = (P + 255) / 256;
	GeomState g;
	g.rec = c.take<float4>(P * BSR_REC);
	g.inst_offset = c.take<uint32_t>(P);
	g.wg_kept = c.take<uint32_t>(n_wg);
	g.wg_area = c.take<uint32_t>(n_wg);
	g.hist1 = c.take<uint32_t>(BSR_RADIX_BINS_ * hist1_columns(n_wg) + 512);   // rows + digit totals + digit bases
	g.kept_mask = c.take<uint64_t>(P);
	g.rect = c.take<ushort4>(P);
	g.clamped = c.take<uint8_t>(P);
	g.depth = c.take<float>(P);
	return g;
}
inline size_t GeomState::bytes(size_t P) { Carver c{nullptr}; layout(c, P); return c.off + 256; }
inline GeomState GeomState::carve(char* p, size_t P) { Carver c{(char*)align_up((size_t)p, 256)}; return layout(c, P); }

// The backward's slab (sized at 40 B per instance + 16: its rows are 36 B, 40 B with the depth gradient, and the
// reader's last 16-byte load of a run may reach 12 B past it) lives in the caller's binning buffer too, over the radix ping-pong
// buffers, which are dead once the forward has returned: the library owns no device memory, as in the reference,
// where every byte of scratch comes from the caller's resize callbacks (rasterize_points.cu:27-33).
// with_slab = false (view-batched forward: inference only) sizes the section for the ping-pong buffers alone.
inline BinState BinState::layout(Carver& c, size_t R, bool with_slab)
{
	BinState b;
	b.point_list = c.take<uint32_t>(R);
	Carver pingpong = c, slab = c;   // the same bytes, laid out twice
	b.elems_a = pingpong.take<BinElem>(R);
	b.elems_b = pingpong.take<BinElem>(R);
	b.slab = (float4*)slab.take<char>(with_slab ? R * BSR_SLAB_ROW_BYTES + BSR_SLAB_TAIL_BYTES : 0);
	c.off = pingpong.off > slab.off ? pingpong.off : slab.off;
	b.hist = c.take<uint32_t>(BSR_RADIX_BINS_ * (BSR_HIST_BLOCKS_MAX + 1));
	return b;
}
inline size_t BinState::bytes(size_t R, bool with_slab) { Carver c{nullptr}; layout(c, R, with_slab); return c.off + 256; }
inline BinState BinState::carve(char* p, size_t R, bool with_slab) { Carver c{(char*)align_up((size_t)p, 256)}; return layout(c, R, with_slab); }

// The backward is handed R, not the capacity the forward carved with: it finds point_list at the buffer's start and
// puts its slab (up to 40 B per KEPT instance) right behind point_list[R].  A buffer carved for `cap` instances serves
// it only if that R-based carve ends inside it -- with kept <= cap < R the slab could otherwise run past the end
// (cap + 512 Ki < R is enough to get past the 2 MB of histogram space behind the work section).
static inline bool backward_fits(size_t cap, size_t R, size_t kept)
{
	Carver c{nullptr};
	c.take<uint32_t>(R);
	c.take<char>(kept * BSR_SLAB_ROW_BYTES + BSR_SLAB_TAIL_BYTES);
	return c.off <= BinState::bytes(cap, true) - 256;
}

inline ImgState ImgState::layout(Carver& c, size_t N, size_t T)
{
	ImgState i;
	i.final_T = c.take<float>(N);
	i.n_contrib = c.take<uint32_t>(N);
	i.tile_range = c.take<uint2>(T);
	i.flags = c.take<int>(BSR_FLAGS_BYTES / sizeof(int));
	i.big_tiles = c.take<uint32_t>(3 * T);
	return i;
}
inline size_t ImgState::bytes(size_t N, size_t T) { Carver c{nullptr}; layout(c, N, T); return c.off + 256; }
inline ImgState ImgState::carve(char* p, size_t N, size_t T) { Carver c{(char*)align_up((size_t)p, 256)}; return layout(c, N, T); }

}  // namespace bsr
