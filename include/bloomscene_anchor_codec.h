/*
 * bloomscene_anchor_codec.h -- C ABI of the anchor position coder: the one stream of a compressed BloomScene scene the
 * reference never writes.  GaussianModel.conduct_encoding (scene/gaussian_model.py:1112, "GM") pickles _anchor, 96 bits
 * an anchor, and reports N * 3 * anchor_round_digits = 48 (GM:1049, GM:1187); the 16-bit lattice indices Quantize_anchor
 * computes (utils/encodings.py:215-227, "ENC") are never written.  Here they are: sorted, and their gaps coded with a
 * per-chunk Golomb-Rice rule.  The decoder returns get_anchor's values bit for bit, which the context model of every other
 * stream (calc_interp_feat -> mlp_grid) is a function of: the anchors are decoded first.
 *
 * THE FORMAT IS OUR OWN: a stream written here is read here.
 *
 * Boundary rules are those of bloomscene_codec.h: plain DEVICE pointers and ints, a hipStream_t passed as void*, 0 on
 * success, bsr_last_error() on failure, no device allocation (the stream and every byte of scratch are the caller's), no
 * state kept between calls, nothing read on the host: the calls only enqueue.  What a call has to tell the host goes to
 * the caller's two `result` words on the DEVICE (status bits, then the stream's length in bytes), which the caller reads
 * once.  No float atomics; the only atomics are integer or (the status word in global memory, a chunk's code words in
 * LDS: order-independent).  A stream is bit-identical from run to run.  Purely additive: BSR_VERSION stays 4.
 *
 * THE LATTICE.  For anchor row r and axis c, with (min, max) = (bound_min, bound_max):
 *   interval_c and q are EXACTLY rule A of bloomscene_anchor_state.h (torch's floating floor-division sequence, clamped to
 *   [0, 65535]); the device function is the same one (csrc/anchor_lattice.h).
 *   A NaN or infinite coordinate, or bounds that give no finite q, set BSR_ANCHOR_CODEC_BAD_VALUE.
 *   key = x << 32 | y << 16 | z with (x, y, z) = (q_0, q_1, q_2): 48 bits, the packed order of bloomscene_voxelize.h and of
 *   np.unique(axis = 0).
 *   decoded anchor[c] = float(q_c) * interval_c + min_c   (two roundings, no contraction): the bits get_anchor and
 *   bsr_anchor_visible_forward return.
 *
 * THE ORDER.  Rows are coded in ascending key, ties in ascending SOURCE row.  bsr_anchor_keys writes the keys in the row
 * list's order; the CALLER sorts them by (key, source row) -- a stable sort by key of a list in ascending row order: the
 * permutation is a pure function of the keys and rows -- and hands the sorted keys to bsr_anchor_codec_encode, which
 * refuses keys that descend (the stream does not depend on how ties were broken; the permutation does).  Equal keys
 * are legal: they code a gap of 0.  The caller applies the permutation to every per-anchor tensor before it codes the
 * attributes.
 *
 * THE CODE.  Keys go in chunks of B = 256 consecutive keys.  For a chunk with m keys:
 *   k = 0 if m < 2;  else mean = (last - first) / (m - 1) (integer division), k = mean == 0 ? 0 : bitlength(mean) - 1
 *   a gap d = key_i - key_(i-1), 0 < i < m, has qh = d >> k and is written as
 *     qh < 32:   qh one-bits, a zero bit, then the k low bits of d (lowest first)
 *     else       32 one-bits, then all 48 bits of d (lowest first)                       (the escape)
 *   Bits are LSB-first inside little-endian 32-bit words.  A gap costs at most 80 bits, a chunk's gaps at most 2552 bytes.
 *
 * STREAM LAYOUT, little endian.
 *   header, 12 uint32: magic 0x41525342 ("BSRA"), format 1, n, chunk count = ceil(n / B), B = 256, the escape length 32,
 *                      min[3] and max[3] as fp32 bit patterns
 *   uint32 offsets[chunk count + 1]: byte offset of each chunk from the end of this table, and the total
 *   per chunk: one uint64 (first key | k << 48; as two uint32, low first: a chunk is 4-byte aligned), then the gap bits
 *              padded with zero bits to a multiple of 4 bytes
 * n == 0 is a header-only stream: chunk count 0, no offset table, 48 bytes.
 *
 * REFUSALS.  Status bits in result[0]; the length is 0 then and the outputs are unspecified (always inside their buffers).
 * The decoder checks every offset against the bytes the caller says the stream has and every word it reads against its
 * chunk's end; a chunk must use its bits exactly up to the padding, the padding must be zero, k must be the one the rule
 * gives for the decoded first and last key, and an escape must be one the rule calls for.  THE FORMAT CARRIES NO CHECKSUM:
 * damage confined to the low bits of a gap decodes to other keys without a status.
 *
 * (Entry point names carry no digits: the header / ctypes table check of tests/test_host_cpu.py reads names as
 * bsr_[a-z_]+.)
 */
#ifndef BLOOMSCENE_ANCHOR_CODEC_H_INCLUDED
#define BLOOMSCENE_ANCHOR_CODEC_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSR_ANCHOR_CODEC_MAGIC 0x41525342u
#define BSR_ANCHOR_CODEC_FORMAT 1
#define BSR_ANCHOR_CODEC_HEADER_BYTES 48
#define BSR_ANCHOR_CODEC_CHUNK 256          /* B */
#define BSR_ANCHOR_CODEC_ESCAPE 32
#define BSR_ANCHOR_CODEC_CHUNK_BYTES 2560   /* the most a chunk takes: 8 + 4 * ceil(255 * 80 / 32) */
#define BSR_ANCHOR_CODEC_MAX_N (1 << 27)    /* the worst-case stream stays below 2^32 bytes: the offsets are uint32 */

/* status bits of result[0] */
#define BSR_ANCHOR_CODEC_BAD_VALUE 1u     /* a non-finite coordinate, or bounds that give no finite lattice index */
#define BSR_ANCHOR_CODEC_BAD_ROW 2u       /* a row of the row list outside [0, N) */
#define BSR_ANCHOR_CODEC_BAD_ORDER 4u     /* encoder: keys that are not ascending */
#define BSR_ANCHOR_CODEC_BAD_KEY 8u       /* a key of 2^48 or more (handed to the encoder, or reached by the decoder) */
#define BSR_ANCHOR_CODEC_BAD_HEADER 16u   /* decoder: wrong magic, format, B, escape length, n or chunk count; bounds not finite */
#define BSR_ANCHOR_CODEC_TRUNCATED 32u    /* decoder: the stream ends before its header, its offset table or a chunk does */
#define BSR_ANCHOR_CODEC_CORRUPT 64u      /* decoder: offsets out of order or misaligned; a code that runs past its chunk's
                                             end; bits not used up to the padding, or padding that is not zero; a k or an
                                             escape the rule does not give */

/* Worst-case bytes of a stream of n anchors (0 for n < 0 or n > BSR_ANCHOR_CODEC_MAX_N). */
size_t bsr_anchor_codec_stream_bound(int n);
/* Bytes of scratch bsr_anchor_codec_encode needs: one byte count per chunk (a multiple of 256, never 0 for a supported n;
 * 0 for an unsupported one).  The other calls need none. */
size_t bsr_anchor_codec_scratch_bytes(int n);

/* The lattice / key pass.
 *   anchor, anchor_stride    _anchor: row r at anchor + r * anchor_stride (>= 3) floats, N rows
 *   bound_min, bound_max     [3] floats on the device
 *   rows                     [n] int64 rows of _anchor to take, in this order; NULL: rows 0 .. n - 1 (then n <= N)
 *   keys                     [n] uint64, fully written (0 for a row that is refused), 8-byte aligned
 *   result                   2 uint32 on the device: status bits (BAD_VALUE, BAD_ROW), then 0 */
int bsr_anchor_keys(int N, int n, const float* anchor, long long anchor_stride, const float* bound_min, const float* bound_max,
                    const long long* rows, unsigned long long* keys, unsigned* result, void* hip_stream);

/* Sorted keys -> the stream.
 *   keys                     [n] uint64, ascending, each below 2^48
 *   bound_min, bound_max     [3] floats on the device: they go into the header
 *   stream                   at least bsr_anchor_codec_stream_bound(n) bytes (stream_bytes says how many), 4-byte aligned
 *   result                   2 uint32 on the device.  result[0] is NOT cleared: the status bits are or-ed into what it
 *                            holds, so that the words bsr_anchor_keys wrote can be handed on and read once (else the
 *                            caller sets it to 0).  result[1]: the stream's length in bytes, 0 with any status bit
 *   scratch                  bsr_anchor_codec_scratch_bytes(n) bytes, 4-byte aligned, contents ignored on entry */
int bsr_anchor_codec_encode(int n, const unsigned long long* keys, const float* bound_min, const float* bound_max,
                            unsigned char* stream, size_t stream_bytes, unsigned* result, void* scratch, void* hip_stream);

/* The stream -> anchor [n, 3] fp32 dense, and optionally the keys and the bounds.
 *   n                        the anchors the caller has room for: a header that says otherwise is BAD_HEADER
 *   stream                   stream_bytes bytes, 4-byte aligned; nothing beyond them is read
 *   keys                     [n] uint64 (8-byte aligned) or NULL
 *   bounds                   6 floats, min[3] then max[3] as the header has them, or NULL
 *   result                   2 uint32 on the device: status bits, then 0 */
int bsr_anchor_codec_decode(int n, const unsigned char* stream, size_t stream_bytes, float* anchor, unsigned long long* keys,
                            float* bounds, unsigned* result, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
