// The cross-lane sum networks of the backward walks: hand-scheduled DPP / permlane sequences, each written once.
//   wave_sums_masked   9 (10) values over the wave's 64 lanes      k_render_bwd_strict, once per visit
//   row8_sums          9 (10) values over every 8-lane group       k_render_bwd_t, NS = 1, once per chunk
//   row4_sums          9 (10) values over every quad               k_render_bwd_t, NS = 2, once per chunk
// The nine- and ten-value forms share their instruction text (string fragments); only the operand lists differ.
// Inline asm gets no automatic wait states: a DPP / permlane read needs 2 after a VALU write of the same VGPR -- the
// orders below keep >= 2 instructions between, s_nop where they cannot.  tests/test_bwd_sums_gpu.py pins which lane
// ends with which sum (through tests/native/pure_functions.hip).
#pragma once
#include "common.h"

namespace bsr {

// one lane-masked (or plain) DPP add: %D (+)= %S from the lanes CTRL names
#define BSR_DPP_ADD(D, S, CTRL) "v_add_f32_dpp %" #D ", %" #S ", %" #S " " CTRL "\n"
#define BSR_DPP_ALL " row_mask:0xf bank_mask:0xf"
// CTRL applied to the accumulators %0..%3 in place / to %0..%3 from four other operands
#define BSR_DPP_ADD4(CTRL) BSR_DPP_ADD(0, 0, CTRL) BSR_DPP_ADD(1, 1, CTRL) BSR_DPP_ADD(2, 2, CTRL) BSR_DPP_ADD(3, 3, CTRL)
#define BSR_DPP_ADD4_FROM(S0, S1, S2, S3, CTRL)                                                                          \
	BSR_DPP_ADD(0, S0, CTRL) BSR_DPP_ADD(1, S1, CTRL) BSR_DPP_ADD(2, S2, CTRL) BSR_DPP_ADD(3, S3, CTRL)

// ---- halving reduction of 9 (10) values over the 64 lanes: lane-masked DPP writes ------------
// Nine independent 6-step reductions would be 54 cross-lane adds.  Instead the values are split
// between partner lanes at every step, halving the live set; a first version selected the kept value
// per lane (2 selects + 1 DPP add per pair, 33 instructions).  Measured on MI355X
// (tools/microbench/valu_rates.hip, 8 waves/SIMD): v_fma/v_mul issue every ~2.6 cycles per SIMD, but
// v_cndmask (SGPR mask), v_cmp -> SGPR and every DPP add every ~4.3.  So the halving steps run over the lane
// bits whose DPP writes the hardware can mask -- bit 2 and 3 through bank_mask (banks of 4 lanes),
// bit 4 and 5 through v_permlane16/32_swap of a PAIR (swap, then one add) -- so a pair-step costs 2
// instructions and no select; the plain steps over bits 0 and 1 come last, on the single survivor.
// 24 instructions for 9 values (25 for 10) instead of 33 (35), in place in the input registers.
// Which lane ends with which component is not assumed: calibrate_components() runs the reduction once
// on constants and reads the mapping off the result.
// All ten values are declared in/out so that no two of them can be given the same register (two inputs
// holding the same SSA value otherwise could, and the block overwrites x0..x3, x8 in place).
// Operands: %0..%3 = x0..x3, %4 = x8, %5 = a temporary, %6..%9 = x4..x7, %10 = x9 (ten values only).
// The step over lane bit 2 pairs x0..x3 with x4..x7; x8 pairs with x9, or alone is summed unmasked.
#define BSR_WSM_BIT2_LO "s_nop 1\n" BSR_DPP_ADD4("row_ror:4 row_mask:0xf bank_mask:0x5")
#define BSR_WSM_BIT2_HI BSR_DPP_ADD4_FROM(6, 7, 8, 9, "row_ror:4 row_mask:0xf bank_mask:0xa")
#define BSR_WSM_REST                                                                                                     \
	BSR_DPP_ADD(0, 0, "row_ror:8 row_mask:0xf bank_mask:0x3")                                                            \
	BSR_DPP_ADD(1, 1, "row_ror:8 row_mask:0xf bank_mask:0x3")                                                            \
	BSR_DPP_ADD(0, 2, "row_ror:8 row_mask:0xf bank_mask:0xc")                                                            \
	BSR_DPP_ADD(1, 3, "row_ror:8 row_mask:0xf bank_mask:0xc")                                                            \
	BSR_DPP_ADD(4, 4, "row_ror:8" BSR_DPP_ALL)                                                                           \
	"v_mov_b32 %5, %4\n"                                                                                                 \
	"v_permlane16_swap_b32 %0, %1\n"                                                                                     \
	"v_add_f32 %0, %0, %1\n"                                                                                             \
	"v_permlane16_swap_b32 %4, %5\n"                                                                                     \
	"v_add_f32 %4, %4, %5\n"                                                                                             \
	"s_nop 1\n"                                                                                                          \
	"v_permlane32_swap_b32 %0, %4\n"                                                                                     \
	"v_add_f32 %0, %0, %4\n"                                                                                             \
	"s_nop 1\n"                                                                                                          \
	BSR_DPP_ADD(0, 0, "quad_perm:[1,0,3,2]" BSR_DPP_ALL)                                                                 \
	"s_nop 1\n"                                                                                                          \
	BSR_DPP_ADD(0, 0, "quad_perm:[2,3,0,1]" BSR_DPP_ALL)
template <bool TEN>
__device__ __forceinline__ float wave_sums_masked(float x0, float x1, float x2, float x3, float x4, float x5, float x6,
                                                  float x7, float x8, float x9)
{
	float t;
	if (TEN) {
		asm volatile(BSR_WSM_BIT2_LO BSR_DPP_ADD(4, 4, "row_ror:4 row_mask:0xf bank_mask:0x5")
		             BSR_WSM_BIT2_HI BSR_DPP_ADD(4, 10, "row_ror:4 row_mask:0xf bank_mask:0xa") BSR_WSM_REST
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x8), "=&v"(t), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x9));
	} else {
		asm volatile(BSR_WSM_BIT2_LO BSR_WSM_BIT2_HI BSR_DPP_ADD(4, 4, "row_ror:4" BSR_DPP_ALL) BSR_WSM_REST
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x8), "=&v"(t), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7));
	}
	(void)t;
	return x0;
}
#undef BSR_WSM_BIT2_LO
#undef BSR_WSM_BIT2_HI
#undef BSR_WSM_REST

// Component (0..NV-1) whose wave total this lane holds after wave_sums_masked, and whether this lane is
// the one that stores it (the lowest lane holding that component).  Sums of small integers are exact.
template <bool TEN>
__device__ __forceinline__ int calibrate_components(int lane, bool& stores)
{
	const float r = wave_sums_masked<TEN>(0.f, 1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f, 9.f);
	const int comp = (int)(r * (1.0f / 64.0f));
	stores = false;
#pragma unroll
	for (int c = 0; c < (TEN ? 10 : 9); c++) {
		const uint64_t m = wave_ballot(comp == c);
		if (comp == c) stores = (m != 0ull) && (lane == (int)__builtin_ctzll(m));
	}
	return comp;
}

// Sum over the 8 lanes sharing (lane >> 3) of nine (ten) values.  On return, in every lane with bit 2 clear x0..x3 (x4
// with TEN) hold the totals of inputs 0..3 (0..4) and x8 that of input 8; in lanes with bit 2 set x0..x3 (x4) hold the
// totals of inputs 4..7 (5..9).  Step over lane bit 2 = halving on bank-masked row rotations (rotate by 12 = "from
// lane + 4" into banks 0 and 2, rotate by 4 = "from lane - 4" into banks 1 and 3: both stay inside the 8-lane group), steps
// over bits 1 and 0 = plain quad permutes.  19 (20) instructions.
// A = the fifth accumulator (x4 of ten values; x8 of nine, which has no partner), S0..S3 = the partners of %0..%3.
#define BSR_ROW8_LO(A)                                                                                                   \
	"s_nop 1\n" BSR_DPP_ADD4("row_ror:12 row_mask:0xf bank_mask:0x5") BSR_DPP_ADD(A, A, "row_ror:12 row_mask:0xf bank_mask:0x5")
#define BSR_ROW8_HI(S0, S1, S2, S3) BSR_DPP_ADD4_FROM(S0, S1, S2, S3, "row_ror:4 row_mask:0xf bank_mask:0xa")
#define BSR_ROW8_QUAD(A)                                                                                                 \
	BSR_DPP_ADD4("quad_perm:[2,3,0,1]" BSR_DPP_ALL) BSR_DPP_ADD(A, A, "quad_perm:[2,3,0,1]" BSR_DPP_ALL)                 \
	BSR_DPP_ADD4("quad_perm:[1,0,3,2]" BSR_DPP_ALL) BSR_DPP_ADD(A, A, "quad_perm:[1,0,3,2]" BSR_DPP_ALL)
template <bool TEN>
__device__ __forceinline__ void row8_sums(float& x0, float& x1, float& x2, float& x3, float& x4, float& x5, float& x6,
                                          float& x7, float& x8, float& x9)
{
	if (TEN) {
		asm volatile(BSR_ROW8_LO(4) BSR_ROW8_HI(5, 6, 7, 8) BSR_DPP_ADD(4, 9, "row_ror:4 row_mask:0xf bank_mask:0xa") BSR_ROW8_QUAD(4)
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x8), "+v"(x9));
	} else {
		asm volatile(BSR_ROW8_LO(8) BSR_ROW8_HI(4, 5, 6, 7) BSR_ROW8_QUAD(8)
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x8), "+v"(x9));
	}
}
#undef BSR_ROW8_LO
#undef BSR_ROW8_HI
#undef BSR_ROW8_QUAD

// NS = 2: the 8 lanes of a slot hold TWO entries (rows 0-3 | rows 4-7): the sums stop at the quad.  On return every
// lane holds the totals of its quad (its half of the slot) in all nine (ten) registers.  18 (20) instructions.
#define BSR_QSTEP(P)                                                                                                     \
	BSR_DPP_ADD4("quad_perm:" P BSR_DPP_ALL) BSR_DPP_ADD(4, 4, "quad_perm:" P BSR_DPP_ALL)                               \
	BSR_DPP_ADD(5, 5, "quad_perm:" P BSR_DPP_ALL) BSR_DPP_ADD(6, 6, "quad_perm:" P BSR_DPP_ALL)                          \
	BSR_DPP_ADD(7, 7, "quad_perm:" P BSR_DPP_ALL) BSR_DPP_ADD(8, 8, "quad_perm:" P BSR_DPP_ALL)
template <bool TEN>
__device__ __forceinline__ void row4_sums(float& x0, float& x1, float& x2, float& x3, float& x4, float& x5, float& x6,
                                          float& x7, float& x8, float& x9)
{
	if (TEN) {
		asm volatile("s_nop 1\n" BSR_QSTEP("[2,3,0,1]") BSR_DPP_ADD(9, 9, "quad_perm:[2,3,0,1]" BSR_DPP_ALL)
		             BSR_QSTEP("[1,0,3,2]") BSR_DPP_ADD(9, 9, "quad_perm:[1,0,3,2]" BSR_DPP_ALL)
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x8), "+v"(x9));
	} else {
		asm volatile("s_nop 1\n" BSR_QSTEP("[2,3,0,1]") BSR_QSTEP("[1,0,3,2]")
		             : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7), "+v"(x8), "+v"(x9));
	}
}
#undef BSR_QSTEP
#undef BSR_DPP_ADD4_FROM
#undef BSR_DPP_ADD4
#undef BSR_DPP_ALL
#undef BSR_DPP_ADD

}  // namespace bsr
