/*
 * cray_hip_exr.h — the C-ABI of libcray_hip_exr.so, the companion library of the output codecs: what leaves the product as a file and needs no scene, no path
 * state and nothing of the render path. Its second codec is the 8-bit frame as a PNG file (crx_png_pack, below), optionally through a display transform — exposure, a tone curve, a dither
 * (crx_png_pack_display) — at an exposure the device can measure from the frame (crx_auto_exposure). Beside the codecs, because it needs no scene either: the firefly
 * filter in front of the denoisers (crx_despeckle). Its first: the pixel data of a ZIP- or ZIPS-compressed scanline OpenEXR file, deflated on the device
 * from the buffers libcray_hip.so already makes (c-ray_amd/csrc/exr_zip.h) — all FLOAT (crx_pack_zip), or with a pixel type per channel, FLOAT or HALF (crx_pack). Plain C, int return codes: 0 (CRH_OK) is ok, the negative CRH_ERR_* values of cray_hip.h
 * are reused, crx_last_error() holds the text of the calling thread's last failure. There is NO CPU path: without a HIP device crx_context_create answers
 * CRH_ERR_NO_DEVICE. A context belongs to one device and one stream and is used by one thread at a time.
 *
 * Why a library of its own: libcray_hip.so is held under 3 MiB (tests/test_abi.py) and is full; nothing in here is needed to render.
 */
#ifndef CRAY_HIP_EXR_H
#define CRAY_HIP_EXR_H

#include <stdint.h>

#include "cray_hip.h"          /* crh_pack_channel, CRH_PACK_MAX_CHANNELS, CRH_OK, CRH_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct crx_ctx crx_ctx;

/* `stream` is a raw hipStream_t (the launches and copies of every call queue behind whatever is on it) or NULL for a stream of the library's own. The scratch of
 * the calls — transformed chunks, segment outputs, the compacted result, the id maps, pinned memory for the copy out — belongs to the context: grown on demand,
 * freed by crx_context_destroy. CRH_ERR_INVALID: out == NULL, device < 0 or not below the device count. */
int crx_context_create(int device, void *stream, crx_ctx **out);
int crx_context_destroy(crx_ctx *ctx);
const char *crx_last_error(void);

/* crh_pack_scanlines' pixel data (cray_hip.h), compressed: the chunks of a scanline OpenEXR file of compression 2 (ZIPS, lines_per_chunk 1) or 3 (ZIP, 16).
 *
 * Channels mean exactly what they mean to crh_pack_scanlines: one component of a device buffer of 32-bit words [H, W, stride], copied bit for bit; with a map the
 * value is an id and the word is map_host[id], 0x00000000 for -1, a fraction, a NaN, or an id at or past map_count. The maps are read before the call returns. The
 * caller guarantees that the sources are complete (after work of another context or stream: synchronise that first).
 *
 * Chunks. A chunk is lines_per_chunk consecutive stored rows starting at a multiple of lines_per_chunk; the image's last chunk may be shorter. first_row must be a
 * multiple of lines_per_chunk, first_row + row_count must be `height` or a multiple of lines_per_chunk.
 * Raw bytes. A chunk's raw bytes R are its rows' planes exactly as crh_pack_scanlines lays them out, without the per-row 8-byte headers:
 * n = 4 * channel_count * width * lines of them.
 * Transform (OpenEXR's ZIP rule). T[i / 2] = R[i] for even i, T[(n + 1) / 2 + i / 2] = R[i] for odd i; then T'[0] = T[0] and T'[j] = (T[j] - T[j - 1] + 128) mod 256
 * for j >= 1, computed on the un-predicted T.
 * The chunk in host_out: int32 y (its first stored row), int32 size, `size` bytes of data. The data is a zlib stream of T' — header 0x78 0x01, deflate blocks any
 * inflate accepts (fixed Huffman codes, or per segment dynamic ones under crx_set_codes below; matches within segments of the chunk), Adler-32 of T' big-endian — if that stream is shorter than n; otherwise the n raw
 * bytes R. size == n means raw. Chunks stand back to back in row order; chunk_bytes_host[k] = 8 + size of chunk k, *total_bytes their sum. host_out must hold
 * 8 * chunks + 4 * channel_count * width * row_count bytes, chunk_bytes_host one entry per chunk; the output is never larger.
 * Determinism. The bytes are a function of the arguments, the sources and of the codes setting (crx_set_codes) only — not of scheduling, of the number of CUs, or of earlier calls: two calls give equal
 * bytes, and the chunks of consecutive calls over first_row ranges concatenate to those of one call.
 * CRH_ERR_INVALID: everything crh_pack_scanlines refuses (a NULL context, list, source or output; channel_count outside 1 .. CRH_PACK_MAX_CHANNELS; a size <= 0; rows
 * outside the image; stride outside 1 .. 64; component >= stride; map_count > 65536; a map with count 0), lines_per_chunk not 1 or 16, misaligned rows, a NULL
 * chunk_bytes_host or total_bytes, a chunk of 2^31 bytes or more. row_count == 0 is CRH_OK, writes nothing and sets *total_bytes to 0. A refused call writes
 * nothing anywhere.
 * The call launches behind whatever is queued on the context's stream, copies the sizes and then `total` bytes through the context's pinned scratch and waits. */
int crx_pack_zip(crx_ctx *ctx, const crh_pack_channel *channels, uint32_t channel_count, int width, int height, int first_row, int row_count, int lines_per_chunk,
                 void *host_out, uint64_t *chunk_bytes_host, uint64_t *total_bytes);

/* crx_pack_zip with a pixel type per channel and the file's compression attribute in place of lines_per_chunk: the pixel data of a scanline OpenEXR file whose
 * colour-like channels are HALF, uncompressed (0), ZIPS (2) or ZIP (3). pixel_types[i] is the type of channels[i]; NULL means all FLOAT.
 *
 * The conversion, part of the interface: binary32 -> binary16, round to nearest, ties to even, in integer arithmetic (c-ray_amd/csrc/exr_zip.h: zipHalfBits), the
 * bits of numpy's astype(float16): gradual underflow to half subnormals; |x| < 2^-25 and the tie 2^-25 itself go to +-0; results that round to 2^16 or more
 * (|x| >= 65520) become +-infinity — values above 65504 do not survive a HALF channel, that is the format —; +-infinity stay; a NaN becomes
 * sign | 0x7c00 | (mantissa >> 13), with bit 0 set if that mantissa field would be 0. HALF on a channel that has a map is refused: an id is a 32-bit word.
 *
 * Raw bytes. A stored row is one plane per channel in list order, `width` pixels of that channel's type each (a HALF pixel: 2 bytes little-endian) — the OpenEXR
 * scanline layout —: rowBytes = width * the sum of the channels' pixel sizes.
 * Chunks. 1 row a chunk for compression 0 and 2, 16 rows for 3, the image's last chunk may be shorter; n = rowBytes * lines, even but not always a multiple of 4.
 * Transform, the choice "zlib stream if shorter than n, else raw", the chunk header int32 y, int32 size, the row alignment rules, determinism and the output bound
 * 8 * chunks + raw bytes (rowBytes * row_count) are crx_pack_zip's with this n. Compression 0 is the chunk form with every chunk raw: int32 y, int32 rowBytes, the
 * row; nothing is transformed or deflated.
 * Identities. With pixel_types NULL or all 0 and compression 2 / 3 the bytes and sizes are those of crx_pack_zip with 1 / 16 lines (the same kernels run); with
 * compression 0 the bytes are those of crh_pack_scanlines.
 * CRH_ERR_INVALID, nothing written anywhere: everything crx_pack_zip refuses, a compression other than 0, 2, 3, a pixel type other than 0 or 1, HALF on a channel
 * with a map, a chunk of 2^31 bytes or more (from rowBytes). */
#define CRX_PIXEL_FLOAT 0          /* the 32-bit word, bit for bit: what crx_pack_zip stores */
#define CRX_PIXEL_HALF 1           /* the word read as binary32, converted to binary16 by the rule above, 2 bytes little-endian */
int crx_pack(crx_ctx *ctx, const crh_pack_channel *channels, const uint8_t *pixel_types, uint32_t channel_count, int width, int height, int first_row, int row_count,
             int compression, void *host_out, uint64_t *chunk_bytes_host, uint64_t *total_bytes);

/* The last complete crx_pack_zip's or crx_pack's kernel time between the library's own events (waits for it): the sum of its launches, and per launch in phases_ms —
 * [0] gather + transform, [1] deflate, [2] sizes and offsets, [3] compaction (compression 0 launches only the last two; the others read 0). 0 before the first call. */
#define CRX_ZIP_PHASES 4
int crx_pack_zip_time_ms(crx_ctx *ctx, float *ms);
int crx_pack_zip_phases_ms(crx_ctx *ctx, float phases_ms[CRX_ZIP_PHASES]);

/* The bytes of T' one deflate segment covers (matches do not cross segments; a chunk of at most this many bytes is one deflate block). */
uint32_t crx_zip_segment_bytes(void);

/* Which Huffman codes the deflate blocks of crx_pack_zip and of crx_pack with compression 2 / 3 use, all FLOAT or with HALF channels (compression 0 deflates
 * nothing and ignores it). The setting is sticky on the context and starts as CRX_CODES_FIXED: the fixed codes of RFC 1951, 3.2.6, the bytes every call wrote before
 * the setting existed. CRX_CODES_DYNAMIC: every segment's block is coded with whichever costs fewer bits — the fixed codes, or a dynamic code (3.2.7) built on the
 * device from that segment's own literal, length and distance counts, none longer than 15 bits (7 for the code-length code); a tie goes to fixed, and a segment
 * that chooses fixed has, bit for bit, the bytes it has under CRX_CODES_FIXED. The parse — which matches are taken — is the same under both settings.
 * A dynamic block is what any inflate accepts: the code-length code is always complete (a second symbol of length 1 where one would do); a segment without a
 * match sends HDIST = 1 with one distance length of 0; a segment whose matches share one distance symbol sends that symbol with length 1.
 * Everything else of the contract stands as it is: the chunk form, the zlib header 78 01, the Adler-32 of T', "stream if shorter than n, else raw" (now on the
 * stream's size under the setting), the output bound, the refusals, the row alignment. A chunk is never larger than under CRX_CODES_FIXED.
 * Determinism: the bytes are a function of the arguments, the sources and of the codes setting only.
 * CRH_ERR_INVALID: a NULL context, a value other than the two (the setting stays as it was); crx_get_codes: a NULL context or output. */
#define CRX_CODES_FIXED 0
#define CRX_CODES_DYNAMIC 1
int crx_set_codes(crx_ctx *ctx, int codes);
int crx_get_codes(crx_ctx *ctx, int *codes);

/* ---- the second codec: the 8-bit frame as a PNG file, filtered and deflated on the device (c-ray_amd/csrc/png_pack.h) ----
 * host_out receives a complete PNG file: the signature; IHDR (8 bits a sample, colour type 2, no interlace); the caller's tEXt chunks, in order; one IDAT; IEND.
 * Every chunk's CRC-32 is in place: no caller needs a CRC or a zlib of its own.
 *
 * Pixels. dev_fb is a frame buffer [H, W, 3] of floats on the context's device, complete (after work of another context or stream: synchronise that first); stored
 * row 0 is the PNG's first row. Byte i of the image is the byte crh_framebuffer_to_srgb8 gives for float i: linearToSRGB, then (unsigned char)min(v * 255, 255) —
 * one statement, c-ray_amd/csrc/srgb8.h, compiled into both libraries. The contract covers finite inputs >= 0, values above 1 included: what a frame holds.
 * Filtered data F. Per row one filter-type byte, then 3 W bytes filtered with bpp = 3 by the PNG specification's rules — 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth —;
 * bytes left of the row and the row above the first row count as 0, arithmetic is mod 256. n = (3 W + 1) H.
 * Adaptive choice (CRX_PNG_FILTER_ADAPTIVE), part of the interface: a row takes the type whose filtered bytes v have the least sum of min(v, 256 - v); ties go to
 * the lowest type number. A fixed `filter` 0 .. 4 uses that type on every row, the first included.
 * IDAT data. A zlib stream of F: header 78 01, deflate blocks any inflate accepts, the big-endian Adler-32 of F. The blocks are crx_pack's segment coder's:
 * segments of crx_zip_segment_bytes() bytes of F, matches never cross a segment; under the context's crx_set_codes setting the fixed codes, or per segment the
 * cheaper of fixed and dynamic.
 * Bound. crx_png_bound gives the worst case for these arguments: the fixed parts and the tEXt chunks, and 4640 bytes for every segment — what a segment without a
 * single match takes under the fixed codes, whose literals from 144 up have 9 bits: there is no stored-block fallback, so noise may come out larger than n, by about
 * an eighth at the most. crx_png_pack refuses a smaller `capacity` and writes nothing; *total_bytes is the file's size, never above the bound.
 * Determinism. The bytes are a function of the arguments, the pixels and the codes setting only.
 * CRH_ERR_INVALID, nothing written anywhere: a NULL context, frame, output or total_bytes (crx_png_bound: a NULL bytes); width or height <= 0, or n >= 2^31; a filter
 * outside -1 .. 4; a NULL text list with a non-zero count; a key that is empty, longer than 79 bytes or NULL, or a NULL value; a capacity below the bound.
 * The call launches behind whatever is queued on the context's stream, copies the size and then the file through the context's pinned scratch and waits. */
#define CRX_PNG_FILTER_ADAPTIVE (-1)          /* 0 .. 4: that PNG filter type on every row */
typedef struct { const char *key, *value; } crx_png_text;          /* a tEXt chunk: Latin-1, key 1 .. 79 bytes */
int crx_png_bound(int width, int height, const crx_png_text *text, uint32_t text_count, uint64_t *bytes);
int crx_png_pack(crx_ctx *ctx, const float *dev_fb, int width, int height, int filter, const crx_png_text *text, uint32_t text_count, void *host_out, uint64_t capacity,
                 uint64_t *total_bytes);
/* The last complete crx_png_pack's kernel time per phase (waits for it): [0] convert, [1] filter (choice and word build), [2] deflate, [3] crc + scan, [4] emit.
 * 0 before the first call. */
#define CRX_PNG_PHASES 5
int crx_png_phases_ms(crx_ctx *ctx, float phases_ms[CRX_PNG_PHASES]);

/* ---- the display transform of the PNG: exposure, a tone curve, an ordered dither (c-ray_amd/csrc/png_display.h) ----
 * crx_png_pack_display is crx_png_pack with an optional transform between the frame's float and the sRGB byte. Everything else of crx_png_pack's contract carries
 * over word for word: the file's form, the filters and the adaptive choice, the IDAT data and the codes setting, crx_png_bound (unchanged), determinism (the bytes are
 * a function of the arguments, the pixels and the codes setting only), tEXt, the copy out. crx_png_phases_ms reports the transform under [0] convert.
 *
 * Per component c of the frame (finite, >= 0, as for crx_png_pack), in float32 arithmetic, in this order of operations, nothing contracted into a fused multiply-add:
 *   x = exposure * c
 *   for every curve but CLAMP: x = x < 1048576.0f ? x : 1048576.0f          (2^20: past it every curve's byte is 255)
 *   CRX_CURVE_CLAMP     y = x                                                (no limit: linearToSRGB8 saturates)
 *   CRX_CURVE_REINHARD  y = (x * (1 + x / (white * white))) / (1 + x)        (extended Reinhard: `white` maps to 1)
 *   CRX_CURVE_ACES      y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)          (the Narkowicz fit)
 *   CRX_CURVE_HABLE     h(v) = (v * (0.15f * v + 0.05f) + 0.004f) / (v * (0.15f * v + 0.5f) + 0.06f) - 0.02f / 0.3f;  y = h(2 * x) / h(2 * white)
 *   t = linearToSRGB(y) * 255.0f                                             (c-ray_amd/csrc/srgb8.h, unchanged)
 * white * white and h(2 * white) are computed once, on the host, by the same float32 statements. No curve gives a NaN, an infinity or a negative value for
 * parameters in range and x <= 2^20. The curves are not strictly monotone in float32: they step down by an ulp or two here and there.
 * The byte. dither == 0: (unsigned char)(t < 255 ? t : 255), crx_png_pack's rule. dither == 1, ordered, 8 x 8:
 *   t' = t + ((float)B(col & 7, row & 7) - 31.5f) / 64.0f;   byte = t' < 0 ? 0 : t' < 255 ? (unsigned char)t' : 255
 * with `row` the stored row, the same offset for the three components of a pixel, and B the Bayer index matrix built bit by bit: for i = 0, 1, 2, bit
 * 2 (2 - i) + 1 of B(x, y) is bit i of x ^ y and bit 2 (2 - i) is bit i of y. B(x, y), one row per y:
 *    0 32  8 40  2 34 10 42
 *   48 16 56 24 50 18 58 26
 *   12 44  4 36 14 46  6 38
 *   60 28 52 20 62 30 54 22
 *    3 35 11 43  1 33  9 41
 *   51 19 59 27 49 17 57 25
 *   15 47  7 39 13 45  5 37
 *   63 31 55 23 61 29 53 21
 * The offset is centred: its mean is 0, so the mean byte of a flat t is t - 0.5, the truncating rule's own; t = 100.25 gives 48 pixels of 100 and 16 of 99 in every
 * 8 x 8 block.
 * Ranges: exposure in [2^-40, 2^40], white in [2^-10, 2^10], both finite; curve one of the four; dither 0 or 1.
 * Identity: with display NULL, or exposure == 1, CRX_CURVE_CLAMP and dither == 0 (whatever `white`), the file is byte for byte crx_png_pack's.
 * CRH_ERR_INVALID, nothing written anywhere and the frame never written: everything crx_png_pack refuses; a curve outside 0 .. 3; an exposure or a white outside its
 * range, or a NaN; a dither other than 0 or 1. */
#define CRX_CURVE_CLAMP 0
#define CRX_CURVE_REINHARD 1
#define CRX_CURVE_ACES 2
#define CRX_CURVE_HABLE 3
typedef struct { float exposure; int curve; float white; int dither; } crx_display;
void crx_display_default(crx_display *d);          /* 1, CRX_CURVE_CLAMP, 4, 0; a NULL d: nothing */
int crx_png_pack_display(crx_ctx *ctx, const float *dev_fb, int width, int height, const crx_display *display /* NULL: the default */, int filter,
                         const crx_png_text *text, uint32_t text_count, void *host_out, uint64_t capacity, uint64_t *total_bytes);

/* An exposure measured from the frame on the device: the one that takes the `permille` / 1000 quantile of the pixels' luminances to `target`.
 *   Luminance per pixel: L = ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b), in float32, in that order.
 *   A pixel counts iff L is finite and > 0. Its bin is bits(L) >> 19 — sign 0, the 8 exponent bits, 4 mantissa bits: sixteen bins an octave, 4 096 bins of uint32,
 *   the largest one in use 4079.
 *   *counted = N, the number of pixels that count. The rank r = (N * permille + 999) / 1000 in 64-bit integers; the key bin k is the smallest bin whose cumulative
 *   count is >= r; *key is the float with the bits (k << 19) | (1 << 18), the bin's midpoint (0.18 lies in bin 1991, whose key is 0.18359375).
 *   *exposure = target / key, one float32 division, then limited to [2^-40, 2^40]. N == 0: *exposure = 1, *key = 0.
 * A percentile, not the log-average: it needs no transcendental function, so it restates bit for bit, and fireflies do not move it.
 * Determinism. Integer counts do not depend on the order they are added in: the result is a function of the pixels and the arguments only — not of scheduling, of
 * the number of CUs, or of earlier calls.
 * CRH_ERR_INVALID, nothing written anywhere: a NULL context, frame, exposure, key or counted; width or height <= 0, or a frame crx_png_pack refuses for its size;
 * permille 0 or above 1000; a target that is a NaN, <= 0 or infinite.
 * The call launches behind whatever is queued on the context's stream and waits; the frame must be complete (as for crx_png_pack). crx_auto_exposure_time_ms: the
 * last complete call's kernel time between the library's own events (waits for it), 0 before the first. */
int crx_auto_exposure(crx_ctx *ctx, const float *dev_fb, int width, int height, uint32_t permille, float target, float *exposure, float *key, uint64_t *counted);
int crx_auto_exposure_time_ms(crx_ctx *ctx, float *ms);

/* ---- the firefly filter: clamp outlier pixels to a rank of their neighbourhood (c-ray_amd/csrc/despeckle.h) ----
 * A path tracer's frame holds a few pixels many times brighter than everything around them. They agree with none of their neighbours, so an edge-aware filter
 * (crh_denoise) keeps them. crx_despeckle measures, per pixel of a guide frame, a scale s in [0, 1] that takes such a pixel down to a limit derived from its
 * neighbours, and multiplies up to 8 frames of the same shape by that one plane, in place. It removes energy: it is opt-in everywhere and is for a filter's input,
 * never for the frame's own file.
 *
 * The rule, part of the interface. All arithmetic is float32, correctly rounded * + / and comparisons in this order, nothing contracted into a fused multiply-add.
 * For every pixel p of dev_guide [H, W, 3]:
 *   1. luminance      L = ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b)
 *   2. bad            p is bad iff any of r, g, b is a NaN or infinite, or L is
 *   3. guarded        g(p) = L if p is not bad and L > 0, otherwise 0
 *   4. neighbours     the pixels q != p with |dx| <= radius and |dy| <= radius that lie inside the image; m of them (bad ones count, with g = 0)
 *   5. effective rank k = min(rank, m)
 *   6. reference      m == 0 (a 1 x 1 image): p is never clamped. Otherwise R = the k-th largest of the g(q), counted with multiplicity (ties need no rule)
 *   7. limit          T = (factor * R) + floor                      (two roundings)
 *   8. clamp          p is clamped iff it is not bad and g(p) > T
 *   9. scale          bad: s(p) = 0;  clamped: s(p) = T / g(p) (one division; below 1, and 0 where T is 0);  otherwise s(p) = 1
 *  10. apply          to every frame: each component becomes c * s(p), one multiplication. Where s(p) == 0 all three components become +0.0f (not c * 0, which
 *                     keeps a sign and turns an infinity into a NaN). Where s(p) == 1 the words stay bit for bit as they are.
 * x -> (factor * x) + floor is monotone in float32, so p is clamped iff fewer than k neighbours have (factor * g(q)) + floor >= g(p): the kernel decides that way
 * and selects R only for a clamped pixel. The statement above stays the contract (tests/despeckle_spec.py restates it in NumPy, bit for bit).
 * What the rule does and does not do. A clamped pixel keeps its colour ratios (one factor for r, g and b). One plane scales several buffers: the half-sample
 * buffer of crh_denoise_variance is the mean of a prefix of the same passes, a per-pixel factor commutes with those means, so scaling the frame and its half by the
 * same s keeps the variance estimate meaningful. rank trades robustness for detail: rank 1 is "no brighter than the brightest neighbour times factor, plus floor";
 * a higher rank tolerates clumps of rank - 1 fireflies, and DIMS A REAL HIGHLIGHT that has fewer than `rank` comparably bright neighbours — a 2 x 2 star on black
 * under the defaults has 3 bright neighbours a pixel, fewer than rank 4, and comes out at `floor`. Lower the rank or raise the floor for such frames.
 * Parameters: radius 1 or 2; rank 1 .. (2 radius + 1)^2 - 1; factor finite in [1, 2^20]; floor finite in [0, 2^20]. crx_despeckle_default: 2, 4, 4, 2^-6.
 * Stats (stats may be NULL): clamped and bad pixels; max_clamped, the largest g(p) of a clamped pixel, 0 if none; min_scale, the smallest s of a clamped pixel, 1 if
 * none.
 * Frames. dev_frames lists frame_count <= 8 device frames [H, W, 3]; frame_count == 0 measures only. The measure launch completes in stream order before any apply
 * launch: dev_guide may itself be among dev_frames (the usual case: the frame is its own guide). A frame listed twice is scaled twice.
 * The plane is scratch of the context, grown on demand; crx_despeckle_scale copies the last complete call's plane [H, W] to host_scale (W * H floats of that call).
 * Determinism. The plane, the frames and the stats are a function of the arguments and the pixels only: the counts are integers, the two float stats a max and a min.
 * CRH_ERR_INVALID, nothing written anywhere: a NULL context or guide; width or height <= 0, or a frame crx_png_pack refuses for its size; a parameter outside its
 * range, or a NaN; frame_count > 8; a NULL list with a non-zero count, or a NULL entry; crx_despeckle_scale: a NULL argument, or no complete call before it.
 * The call launches behind whatever is queued on the context's stream and waits; the guide and the frames must be complete (as for crx_png_pack).
 * crx_despeckle_time_ms: the last complete call's kernel time between the library's own events (waits for it): [0] measure, [1] apply, summed over the frames;
 * 0 before the first. */
typedef struct { int radius; int rank; float factor; float floor; } crx_despeckle_params;
typedef struct { uint64_t clamped, bad; float max_clamped, min_scale; } crx_despeckle_stats;
void crx_despeckle_default(crx_despeckle_params *p);          /* 2, 4, 4, 2^-6; a NULL p: nothing */
int crx_despeckle(crx_ctx *ctx, const crx_despeckle_params *params /* NULL: the default */, const float *dev_guide, int width, int height, float *const *dev_frames,
                  uint32_t frame_count, crx_despeckle_stats *stats);
int crx_despeckle_scale(crx_ctx *ctx, float *host_scale);
int crx_despeckle_time_ms(crx_ctx *ctx, float ms[2]);

/* ---- debug ---- */
/* The code construction of CRX_CODES_DYNAMIC on histograms of the caller's: `count` histograms of `symbols` counts each in freq (host memory), one wave a
 * histogram through the device function the deflate kernel calls (c-ray_amd/csrc/exr_zip.h: zipCodeLengths); lengths[h * symbols + s] is the code length of symbol
 * s under histogram h. A count of zero gives length 0; a used symbol 1 .. limit. Two or more used symbols give a complete prefix code (Kraft sum exactly 1), of
 * Huffman's cost wherever Huffman's tree of least depth stays within the limit. A single used symbol gets length 1 and nothing else gets a length — the one
 * incomplete code inflate allows (for a code-length code the deflate kernel adds a second symbol itself). No used symbol: all zero.
 * CRH_ERR_INVALID: a NULL argument, symbols outside 1 .. 288 or above 2^limit, a limit other than 7 or 15, a histogram whose counts sum to 2^23 or more, 2^20
 * histograms or more. count == 0 is CRH_OK. */
int crx_debug_code_lengths(crx_ctx *ctx, const uint32_t *freq, uint32_t symbols, uint32_t limit, uint32_t count, uint8_t *lengths);
/* The CRC-32 of crx_png_pack's IDAT on bytes of the caller's: n bytes of host memory in pieces of piece_bytes, the last one shorter; one wave a piece takes its
 * register (zero initial value), one workgroup combines the pieces' (register, x^(8 length) mod P) pairs by the scan crx_png_pack runs over its segments, the
 * conditioning applied once at the ends. *crc is what zlib's crc32 gives for the bytes, whatever the pieces; n == 0 gives 0.
 * CRH_ERR_INVALID: a NULL context or crc, NULL bytes with n > 0, piece_bytes == 0, n >= 2^32, 2^28 pieces or more. */
int crx_debug_crc32(crx_ctx *ctx, const void *host_bytes, uint64_t n, uint32_t piece_bytes, uint32_t *crc);

#ifdef __cplusplus
}
#endif
#endif
