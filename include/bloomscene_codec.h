/*
 * bloomscene_codec.h -- C ABI of the entropy codec: what BloomScene's `encoder_gaussian` / `decoder_gaussian` /
 * `encoder` / `decoder` (utils/encodings.py:84-174, "UE") do through torchac, as an interleaved rANS coder on the GPU.
 * No cdf table is built for the Gaussian model: a lane evaluates the two integer cdf values of its own symbol from
 * (mean, scale, Q) where it needs them, and the SAME device function serves the encoder and the decoder, so the decoder's
 * model is the encoder's bit for bit.
 *
 * THE FORMAT IS OUR OWN.  It is NOT byte-compatible with torchac's streams and is not pinned to them (torchac is on none
 * of the machines this project is built or tested on).  A stream written here is read here.
 *
 * Boundary rules are those of bloomscene_entropy.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (the stream and every byte of scratch are the caller's), no
 * state kept between calls, nothing read on the host: the calls only enqueue.  What a call has to tell the host goes to
 * the caller's `result` words on the DEVICE (status, then the stream's length in bytes), which the caller reads once.
 * No float atomics; the only atomics are integer min / max / or.  A stream is bit-identical from run to run.
 * Purely additive: BSR_VERSION stays 4.
 *
 * THE FUNCTION (fp32, source order, no contraction; rint is IEEE round-half-even as torch.round).
 *
 * SYMBOLS.  Operands x, mean, scale are [n, C]; Q is one value, one per row or one per element; the optional `keep` is
 * [n, C / r] and governs column j through keep[i, j / r] (the [m, K, 1] mask of scene/gaussian_model.py:1172-1178 with
 * r = 3): an element whose entry is 0 is SKIPPED.  The coded order is the row-major order of [n, C], skipped ones included.
 *   k = rint(x / Q)                                     (IEEE division)
 *   min, max of k over the elements not skipped         (a first pass; integer atomics);   L = max - min + 1,  j = k - min
 *   decoded value = float(j + min) * Q ;  a skipped element decodes as 0
 *   s = scale < scale_min ? scale_min : scale           (UE's callers clamp at 1e-9: gaussian_model.py:1145-1147)
 *
 * INTEGER MODEL, 16 bits.  M = 65536 - 2 L.
 *   c(0) = 0,  c(L) = 65536,  and for 0 < j < L:   c(j) = rint(Phi(z_j) * float(M)) + 2 j
 *   z_j = ((float(min + j) - 0.5f) * Q - mean) / s
 * Symbol j owns [c(j), c(j + 1)).  Phi is PINNED (Abramowitz-Stegun 7.1.26 for erfc(|z| / sqrt 2) over bsr_expf, the
 * pinned exp of csrc/common.h), operation by operation.  7.1.26 is a polynomial in t = 1 / (1 + 0.3275911 a); it is
 * evaluated in u = 1 - t with the coefficients expanded accordingly (their sum, 0.999999999, is 1.0f), because in t the
 * roundings of 1 + 0.3275911 a and of partial sums near 1.45 cost 3e-7 around z = 0, where u is small and exact enough:
 *   a = |z| * 0.70710678118654752440f ;  a = a > 16.0f ? 16.0f : a       (bsr_expf(-(a * a)) is exactly 0 from a = 10.2 on)
 *   w = 0.3275911f * a ;  u = w / (1.0f + w)
 *   p = -1.061405429f * u + 3.853875118f ;  p = p * u + -6.222859923f ;  p = p * u + 5.874886615f
 *   p = p * u + -3.44449638f ;  p = p * u + 1.0f       (each product rounded, then each sum: no fma)
 *   h = 0.5f * (p * bsr_expf(-(a * a)))
 *   Phi = z < 0 ? h : 1.0f - h
 * Its absolute error, 1.5e-7 (tests/test_codec_cpu.py: below 2e-7 against float64), is far below one count of M.
 * An infinite z (a point mass, s = 1e-9) is legal: Phi is 0 or 1.  z is never a NaN for operands that are not refused.
 * WHY c IS STRICTLY INCREASING.  z_j is non-decreasing in j: float(min + j), the subtraction of 0.5, the product with
 * Q > 0, the subtraction of mean and the division by s > 0 are each monotone fp32 operations.  The formula for Phi is
 * monotone in exact arithmetic; its fp32 rounding noise (a few 1e-8) times M <= 65532 is a small fraction of a count, so
 * rint(Phi * M) falls from one j to the next by at most ONE count.  With the + 2 j term c(j + 1) - c(j) >= 2 - 1 = 1
 * inside, c(1) >= 2 > c(0) and c(L - 1) <= M + 2 L - 2 = 65534 < c(L).  So for 2 <= L <= 32767 (the reference's int16
 * index range) every frequency is in [1, 65535] and the decoder's binary search is valid.  A symbol the model gives no
 * mass still has frequency 2.
 *
 * TABLE MODEL (the second model of the same kernels).  Symbols are the caller's int16 values in [0, L), min = 0, and
 *   c(j) = rint(cdf[i * cs + j] * float(M)) + 2 j   for 0 < j < L,   c(0) = 0,  c(L) = 65536
 * from a caller's float table of L + 1 columns read through the row stride cs; cs == 0 means one row for all elements
 * (the Bernoulli coder of UE:141-174).  A row that is not non-decreasing within [0, 1] (a NaN included) sets the status
 * word.  For a valid row rint(cdf * M) is non-decreasing and c increases by at least 2.
 *
 * CODER.  Interleaved rANS, 32-bit state x in [2^16, 2^32), 16-bit words, start state 2^16.  With f = c(j + 1) - c(j) and
 * b = c(j):
 *   encode:  if x >= f * 2^16: emit (x & 0xffff), x >>= 16      (at most ONE word: x >> 16 < 2^16 <= f * 2^16)
 *            x = (x / f) * 2^16 + (x % f) + b
 *   decode:  v = x & 0xffff ;  j = the symbol with c(j) <= v < c(j + 1) ;  x = f * (x >> 16) + v - b
 *            if x < 2^16: x = x * 2^16 + next word
 * Element i of the coded order belongs to chunk i / (64 T), step (i / 64) mod T, lane i mod 64; one wave owns a chunk.
 * The encoder runs the steps of a chunk in reverse; the lanes that emit in a step are found with one ballot and their words
 * lie side by side in lane order, the steps' groups in step order.  The decoder runs forward: the lanes with x < 2^16
 * after a step take the next words in lane order.  It finds j by a bisection of ceil(log2 L) trips, the same for every
 * lane.  A skipped element leaves its lane's state untouched in that step.  After its last step every lane of a decoding
 * chunk must be back at 2^16; otherwise the stream is corrupt.  Every word read is checked against the chunk's end from
 * the offset table, every offset against the bytes the caller says the stream has: a truncated or corrupt stream sets the
 * status word and decodes to unspecified symbols, and never makes a kernel leave its buffers.
 *
 * STREAM LAYOUT, little endian.
 *   header, 8 uint32: magic 0x43525342 ("BSRC"), format version 1, model kind, coded elements n * C, min (int32), L, T,
 *                     chunk count
 *   uint32 offsets[chunk count + 1]: byte offset of each chunk from the end of this table, and the total
 *   per chunk: 64 uint32 final states (lane order), then its uint16 words in decode order
 * Nothing coded (no element, or every element skipped) is L = 0; L == 1 needs no words: both are header-only streams
 * (chunk count 0, no offset table, 32 bytes).
 *
 * REFUSALS.  Status bits in result[0]; the length is 0 then and the stream's contents are unspecified.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_CODEC_H_INCLUDED
#define BLOOMSCENE_CODEC_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_CODEC_MAGIC 0x43525342u
#define BSR_CODEC_FORMAT 1
#define BSR_CODEC_HEADER_BYTES 32
#define BSR_CODEC_KIND_GAUSSIAN 0
#define BSR_CODEC_KIND_TABLE 1
#define BSR_CODEC_DEFAULT_STEPS 256   /* T: 256 B of final states per 16384 symbols = 1/8 bit per symbol */
#define BSR_CODEC_MAX_SYMBOLS 32767   /* L */
#define BSR_CODEC_MAX_ELEMENTS (1LL << 30)   /* and bsr_codec_stream_bound below 2^32: the offsets are uint32 */

/* q_mode: what q points to (the values of BSR_ENTROPY_Q_*) */
#define BSR_CODEC_Q_SINGLE 0   /* one float */
#define BSR_CODEC_Q_ROW 1      /* [n] floats (BloomScene's [n, 1]) */
#define BSR_CODEC_Q_ELEMENT 2  /* [n, C] floats, dense */

/* status bits of result[0] */
#define BSR_CODEC_BAD_VALUE 1u     /* a non-finite x / Q, or |rint(x / Q)| >= 2^30 */
#define BSR_CODEC_BAD_STEP 2u      /* Q <= 0 or not finite */
#define BSR_CODEC_BAD_MODEL 4u     /* a non-finite mean or scale */
#define BSR_CODEC_BAD_SPAN 8u      /* L > 32767 */
#define BSR_CODEC_BAD_TABLE 16u    /* a table row not non-decreasing within [0, 1] */
#define BSR_CODEC_BAD_SYMBOL 32u   /* table model, encoder: a symbol outside [0, L) */
#define BSR_CODEC_BAD_HEADER 64u   /* decoder: wrong magic, version or kind, or a header that does not fit the operands */
#define BSR_CODEC_TRUNCATED 128u   /* decoder: the stream ends before its header, offset table or a chunk's words do */
#define BSR_CODEC_CORRUPT 256u     /* decoder: offsets out of order, or a lane that does not return to its start state */

/* Worst-case bytes of a stream of `elements` symbols with T steps a chunk: header, offset table, final states and one word
 * per symbol.  0 for an unsupported argument (elements < 0 or > BSR_CODEC_MAX_ELEMENTS, T < 1 or > 65536). */
size_t bsr_codec_stream_bound(long long elements, int T);
/* Bytes of scratch the two encoders need (a multiple of 256; 0 for an unsupported argument).  Opaque: min / max, and per
 * chunk a word count, the final states and the worst-case word area.  The decoders need none. */
size_t bsr_codec_scratch_bytes(long long elements, int T);

/* Gaussian model, encoder.
 *   x, mean, scale   fp32, element (i, j) at p[i * stride + j]: xs, ms, ss >= C are ROW strides in elements (a column block
 *                    of a wider matrix is read in place)
 *   q                fp32, by q_mode;  keep [n, C / r] fp32 dense or NULL (then r must be 1)
 *   T                steps a chunk, 1 .. 65536
 *   stream           at least bsr_codec_stream_bound(n * C, T) bytes (stream_bytes says how many), 4-byte aligned
 *   result           2 uint32 on the device: status bits, then the stream's length in bytes (0 with a status)
 *   scratch          bsr_codec_scratch_bytes(n * C, T) bytes, 8-byte aligned, contents ignored on entry
 * Supported: 0 <= n, 1 <= C, 1 <= r, C % r == 0, n * C <= BSR_CODEC_MAX_ELEMENTS. */
int bsr_codec_encode_gaussian(int n, int C, int r, const float* x, long long xs, const float* mean, long long ms,
                              const float* scale, long long ss, const float* q, int q_mode, const float* keep,
                              float scale_min, int T, unsigned char* stream, size_t stream_bytes, unsigned* result,
                              void* scratch, void* hip_stream);

/* Gaussian model, decoder: out [n, C] fp32 dense, fully written (zeros where nothing can be decoded).
 *   stream           stream_bytes bytes, 4-byte aligned; nothing beyond them is read
 *   result           2 uint32 on the device: status bits, then one word the call uses for itself */
int bsr_codec_decode_gaussian(int n, int C, int r, const unsigned char* stream, size_t stream_bytes, const float* mean,
                              long long ms, const float* scale, long long ss, const float* q, int q_mode,
                              const float* keep, float scale_min, float* out, unsigned* result, void* hip_stream);

/* Table model.  sym / out [n] int16; cdf fp32 with L + 1 columns, row i at cdf + i * cs (cs == 0: one row; else
 * cs >= L + 1 and n rows); 1 <= L <= BSR_CODEC_MAX_SYMBOLS.  The rest as above. */
int bsr_codec_encode_table(int n, int L, const short* sym, const float* cdf, long long cs, int T, unsigned char* stream,
                           size_t stream_bytes, unsigned* result, void* scratch, void* hip_stream);
int bsr_codec_decode_table(int n, int L, const unsigned char* stream, size_t stream_bytes, const float* cdf, long long cs,
                           short* out, unsigned* result, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
