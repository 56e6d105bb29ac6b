// Test-only: the three pieces of device code that stand behind almost every op, each on its own and on given inputs:
//   wg_scan.h     the workgroup prefix sums, counts, totals and the in-place array scan  (tests/test_wg_scan_gpu.py)
//   grid_sum.h    the deterministic last-workgroup fp64 sum and its ticket               (tests/test_grid_sum_gpu.py)
//   mlp_wgrad.*   the weight-gradient sums of the anchor heads and the context head      (tests/test_mlp_wgrad_direct_gpu.py)
// The kernels here only load what the test hands in, call the product's function the way the product's kernels call it
// (the same template arguments, the same LDS alternation) and store what it returned.  tests/native/Makefile compiles
// this file and the product's mlp_wgrad.hip, unchanged, with the product's FLAGS into libbsr_shared_pieces.so.  Every
// entry point returns non-zero on a refused argument or a launch error and never synchronises.  Nothing here is part of
// the product library.
#include "../../bloomscene_amd/csrc/wg_scan.h"
#include "../../bloomscene_amd/csrc/grid_sum.h"
#include "../../bloomscene_amd/csrc/mlp_wgrad.h"
#include <cstdarg>
#include <cstdio>

namespace bsr {

// common.h declares it, host_state.hip defines it for the product; here the message goes to stderr
int fail(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vfprintf(stderr, fmt, ap);
	va_end(ap);
	fputc('\n', stderr);
	return 1;
}

}  // namespace bsr

using namespace bsr;

// ---- wg_scan.h ----

// of the form of binning.hip's Hist1ColumnValid, with its own per and n_wg
struct ColumnValid {
	int per, n_wg;
	__device__ __forceinline__ bool operator()(int col) const { return hist1_wg_of_column(col, per) < n_wg; }
};

// `calls` scans back to back on the same s_wave, as k_scans does: call c on data + c * pitch, writing iff bit c of
// write_mask; every thread records what each call returned -> totals[c][thread]
template <int WAVES, int VPT, typename Valid>
__global__ void __launch_bounds__(64 * WAVES) k_pt_scan(int n, uint32_t* data, size_t pitch, unsigned write_mask, int calls,
                                                        Valid valid, uint32_t* __restrict__ totals)
{
	__shared__ uint32_t s_w[2 * WAVES];
	for (int c = 0; c < calls; c++) {
		const uint32_t total = wg_exclusive_scan<WAVES, VPT, Valid>(n, data + (size_t)c * pitch, s_w, ((write_mask >> c) & 1u) != 0, valid);
		totals[(size_t)c * 64 * WAVES + threadIdx.x] = total;
	}
}

__global__ void k_pt_wg_of_column(int n, int per, int* __restrict__ out)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < n) out[c] = hist1_wg_of_column(c, per);
}

// `rounds` calls in a loop on two alternating LDS sets, as k_voxel_emit does; round k takes in[k][thread] (COUNT: as a
// predicate, != 0) -> out[k][thread], total[k][thread] (with_total == 0: the overload without a total; `total` stays)
template <int WAVES, bool COUNT>
__global__ void __launch_bounds__(64 * WAVES) k_pt_rounds(int rounds, int with_total, const uint32_t* __restrict__ in,
                                                          uint32_t* __restrict__ out, uint32_t* __restrict__ total)
{
	__shared__ uint32_t s_wave[2][WAVES];
	for (int k = 0; k < rounds; k++) {
		const size_t i = (size_t)k * 64 * WAVES + threadIdx.x;
		const uint32_t v = in[i];
		uint32_t t = 0u, r;
		if (with_total) r = COUNT ? wg_exclusive_count<WAVES>(v != 0u, s_wave[k & 1], t) : wg_exclusive_sum<WAVES>(v, s_wave[k & 1], t);
		else r = COUNT ? wg_exclusive_count<WAVES>(v != 0u, s_wave[k & 1]) : wg_exclusive_sum<WAVES>(v, s_wave[k & 1]);
		out[i] = r;
		if (with_total) total[i] = t;
	}
}

// workgroup b asks for counts[0 .. b), as k_decide_plan does, and for the total of its own row of `values`, on the
// LDS set next to it -> of[b][thread], tot[b][thread]
template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_pt_totals(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ values,
                                                          uint32_t* __restrict__ of, uint32_t* __restrict__ tot)
{
	__shared__ uint32_t part[2][WAVES];
	const size_t i = (size_t)blockIdx.x * 64 * WAVES + threadIdx.x;
	of[i] = wg_total_of<WAVES>(counts, (int)blockIdx.x, part[0]);
	tot[i] = wg_total<WAVES>(values[i], part[1]);
}

// ---- grid_sum.h ----

// thread t of workgroup b brings in[(b * 256 + t) * N + k]; the one thread grid_sum returns true to stores the N
// totals and counts itself in `winners`
template <int N>
__global__ void __launch_bounds__(256) k_pt_grid_sum(const double* __restrict__ in, unsigned* ticket, double* psum,
                                                     double* __restrict__ out, unsigned* winners)
{
	double v[N];
#pragma unroll
	for (int k = 0; k < N; k++) v[k] = in[((size_t)blockIdx.x * 256 + threadIdx.x) * N + k];
	if (grid_sum<N, 256>(v, ticket, psum)) {
#pragma unroll
		for (int k = 0; k < N; k++) out[k] = v[k];
		atomicAdd(winners, 1u);
	}
}

// grid_last_ticket twice in a row with two tickets.  Before call c thread 0 stores blockIdx.x + 1 into its word of row
// c; the workgroup the call returns true to adds all words of the row through load_u32 -> out[3 c] += its threads'
// sums, out[3 c + 1] = its index, out[3 c + 2] += 1 (out: zeroes, the index a sentinel)
__global__ void __launch_bounds__(256) k_pt_tickets(unsigned* tickets, unsigned* words, unsigned* out)
{
	for (int c = 0; c < 2; c++) {
		unsigned* row = words + (size_t)c * gridDim.x;
		if (threadIdx.x == 0) row[blockIdx.x] = blockIdx.x + 1u;
		if (grid_last_ticket(&tickets[c])) {
			unsigned s = 0u;
			for (unsigned b = threadIdx.x; b < gridDim.x; b += 256u) s += load_u32(&row[b]);
			atomicAdd(&out[3 * c], s);
			if (threadIdx.x == 0) {
				out[3 * c + 1] = blockIdx.x;
				atomicAdd(&out[3 * c + 2], 1u);
			}
		}
	}
}

extern "C" {

// The instantiations of wg_exclusive_scan in csrc, by number: 0 <16, 4> AllValid, 1 <16, 4> with ColumnValid{per, n_wg},
// 2 <16, 8>, 3 <16, 1>, 4 <4, 1>.  data: calls rows of `pitch` >= n words; totals: calls x 64 * WAVES words.
int pt_wg_scan(int inst, int n, uint32_t* data, size_t pitch, unsigned write_mask, int calls, int per, int n_wg, uint32_t* totals,
               void* stream)
{
	hipStream_t s = (hipStream_t)stream;
	if (n < 0 || calls < 1 || calls > 32 || pitch < (size_t)n) return 1;
	switch (inst) {
	case 0: hipLaunchKernelGGL((k_pt_scan<16, 4, AllValid>), dim3(1), dim3(1024), 0, s, n, data, pitch, write_mask, calls, AllValid(), totals); break;
	case 1:
		if (per < 1) return 1;
		hipLaunchKernelGGL((k_pt_scan<16, 4, ColumnValid>), dim3(1), dim3(1024), 0, s, n, data, pitch, write_mask, calls, ColumnValid{per, n_wg}, totals);
		break;
	case 2: hipLaunchKernelGGL((k_pt_scan<16, 8, AllValid>), dim3(1), dim3(1024), 0, s, n, data, pitch, write_mask, calls, AllValid(), totals); break;
	case 3: hipLaunchKernelGGL((k_pt_scan<16, 1, AllValid>), dim3(1), dim3(1024), 0, s, n, data, pitch, write_mask, calls, AllValid(), totals); break;
	case 4: hipLaunchKernelGGL((k_pt_scan<4, 1, AllValid>), dim3(1), dim3(256), 0, s, n, data, pitch, write_mask, calls, AllValid(), totals); break;
	default: return 1;
	}
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// out[c] = hist1_wg_of_column(c, per) for c < n
int pt_hist1_wg_of_column(int n, int per, int* out, void* stream)
{
	if (n < 1 || per < 1) return 1;
	hipLaunchKernelGGL(k_pt_wg_of_column, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, per, out);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// wg_exclusive_sum<4> (count == 0) / wg_exclusive_count<4>: in, out, total: rounds x 256 words
int pt_wg_rounds(int count, int rounds, int with_total, const uint32_t* in, uint32_t* out, uint32_t* total, void* stream)
{
	if (rounds < 1) return 1;
	if (count) hipLaunchKernelGGL((k_pt_rounds<4, true>), dim3(1), dim3(256), 0, (hipStream_t)stream, rounds, with_total, in, out, total);
	else hipLaunchKernelGGL((k_pt_rounds<4, false>), dim3(1), dim3(256), 0, (hipStream_t)stream, rounds, with_total, in, out, total);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// wg_total_of<4> and wg_total<4>: counts: at least grid - 1 words; values, of, tot: grid x 256 words
int pt_wg_totals(int grid, const uint32_t* counts, const uint32_t* values, uint32_t* of, uint32_t* tot, void* stream)
{
	if (grid < 1) return 1;
	hipLaunchKernelGGL((k_pt_totals<4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, counts, values, of, tot);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// grid_sum<N, 256> for the N the losses use (1, 2, 5).  in: grid x 256 x N doubles; ticket: one word, zeroed here before
// the launch; psum: N * grid doubles; out: N doubles; winners: one zeroed word
int pt_grid_sum(int N, int grid, const double* in, unsigned* ticket, double* psum, double* out, unsigned* winners, void* stream)
{
	hipStream_t s = (hipStream_t)stream;
	if (grid < 1) return 1;
	if (hipMemsetAsync(ticket, 0, sizeof(unsigned), s) != hipSuccess) return 2;
	if (N == 1) hipLaunchKernelGGL((k_pt_grid_sum<1>), dim3(grid), dim3(256), 0, s, in, ticket, psum, out, winners);
	else if (N == 2) hipLaunchKernelGGL((k_pt_grid_sum<2>), dim3(grid), dim3(256), 0, s, in, ticket, psum, out, winners);
	else if (N == 5) hipLaunchKernelGGL((k_pt_grid_sum<5>), dim3(grid), dim3(256), 0, s, in, ticket, psum, out, winners);
	else return 1;
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// tickets: two words, zeroed here; words: 2 x grid; out: 6 words {sum, index, count} x 2, the sums and counts zeroed
int pt_grid_tickets(int grid, unsigned* tickets, unsigned* words, unsigned* out, void* stream)
{
	hipStream_t s = (hipStream_t)stream;
	if (grid < 1) return 1;
	if (hipMemsetAsync(tickets, 0, 2 * sizeof(unsigned), s) != hipSuccess) return 2;
	hipLaunchKernelGGL(k_pt_tickets, dim3(grid), dim3(256), 0, s, tickets, words, out);
	return hipGetLastError() == hipSuccess ? 0 : 2;
}

// (host side: no GPU) mlp_wgrad_layout -> ldx, ldh, ld2, chunks, tot, off_hid, off_dp1, off_dp2, off_partials, floats
void pt_mlp_wgrad_layout(int n, int wx, int wh, int w2, int tot, size_t* out)
{
	const MlpWgradLayout l = mlp_wgrad_layout(n, wx, wh, w2, tot);
	const size_t v[10] = {l.ldx, l.ldh, l.ld2, l.chunks, (size_t)l.tot, l.off_hid, l.off_dp1, l.off_dp2, l.off_partials, l.floats};
	for (int i = 0; i < 10; i++) out[i] = v[i];
}

// The host side of a backward entry point around the sums, as heads.hip and context.hip call it.  Segments: seg_size,
// seg_dst (NULL: not asked for) in table order.  Product i: A = columns a_col[i] .. + J[i] of the row array a_arr[i]
// (0 x, 1 hid, 2 dp1, 3 dp2 of the carved scratch: the rows the test has filled), B likewise, dW at the start of
// segment wseg[i] and db at the start of segment bseg[i] of a partial.  scratch: mlp_wgrad_layout(...).floats floats.
int pt_mlp_wgrad(int n, int wx, int wh, int w2, int n_seg, const int* seg_size, float* const* seg_dst, int n_prod, const int* a_arr,
                 const int* a_col, const int* b_arr, const int* b_col, const int* J, const int* Kd, const int* wseg, const int* bseg,
                 void* scratch, void* stream)
{
	const char* who = "pt_mlp_wgrad";
	hipStream_t st = (hipStream_t)stream;
	if (n < 0 || n_seg < 1 || n_seg > MLP_WGRAD_MAX_SEGMENTS || n_prod < 1 || n_prod > MLP_WGRAD_MAX_PRODUCTS) return 1;
	MlpSegments d = {};
	for (int i = 0; i < n_seg; i++) {
		if (seg_size[i] < 1) return 1;
		d.add(seg_size[i], seg_dst[i]);
	}
	if (mlp_wgrad_check(who, d)) return 1;
	if (!mlp_wgrad_asked(d)) return 0;
	if (n == 0) return mlp_wgrad_zero(who, d, st);
	const MlpWgradLayout l = mlp_wgrad_layout(n, wx, wh, w2, d.tot);
	MlpRowScratch rs;
	if (mlp_wgrad_carve(who, l, true, scratch, rs)) return 1;
	float* const arr[4] = {rs.x, rs.hid, rs.dp1, rs.dp2};
	const size_t ld[4] = {rs.ldx, rs.ldh, rs.ldh, rs.ld2};
	const int width[4] = {wx, wh, wh, w2};
	MlpProducts p = {};
	for (int i = 0; i < n_prod; i++) {
		// (a product the kernels would read or write out of bounds is refused here, not run)
		if (a_arr[i] < 0 || a_arr[i] > 3 || b_arr[i] < 0 || b_arr[i] > 3 || J[i] < 1 || Kd[i] < 1) return 1;
		if (a_col[i] < 0 || a_col[i] + J[i] > width[a_arr[i]] || b_col[i] < 0 || b_col[i] + Kd[i] > width[b_arr[i]]) return 1;
		if (wseg[i] < 0 || wseg[i] >= n_seg || bseg[i] < 0 || bseg[i] >= n_seg) return 1;
		if (d.s[wseg[i]].first + J[i] * Kd[i] > d.tot || d.s[bseg[i]].first + J[i] > d.tot) return 1;
		p.add(arr[a_arr[i]] + a_col[i], ld[a_arr[i]], arr[b_arr[i]] + b_col[i], ld[b_arr[i]], J[i], Kd[i], d, wseg[i], bseg[i]);
	}
	return mlp_wgrad_sums(who, p, d, n, l, scratch, st);
}

}  // extern "C"
