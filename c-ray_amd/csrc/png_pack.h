/*
 * png_pack.h — the kernels of crx_png_pack (include/cray_hip_exr.h): the 8-bit sRGB frame as a complete PNG file, filtered and deflated on the device. The second
 * codec of libcray_hip_exr.so; included by exr_zip.hip behind exr_zip.h, whose deflate (zipDeflate, one wave per segment of CRX_SEG bytes) it reuses as it is.
 *
 * Seven launches on one stream, ordered by launch order alone, in the five phases crx_png_phases_ms reports:
 *   convert   k_png_convert   floats -> the 8-bit image on the device, once (srgb8.h: THE conversion, the bytes of crh_framebuffer_to_srgb8); a lane makes one word.
 *                             crx_png_pack_display with a transform that is not the identity launches png_display.h's k_png_convert_display in its place.
 *   filter    k_png_choose    one wave per row: the five filters' sums of min(v, 256 - v) by wave reductions, the least wins, ties to the lowest type; a fixed
 *                             filter is written as it is. Every row's type in one launch.
 *             k_png_filter    F — per row the type byte, then the 3 W filtered bytes — as whole words, the way k_zip_transform builds T': a lane makes four
 *                             consecutive bytes and stores one word. A row starts at r (3 W + 1), so a word can hold bytes of two rows and a type byte; the bytes
 *                             behind n = (3 W + 1) H in the last word are stored as zero (zipDeflate loads whole words; n may be odd: zipParse takes no position at
 *                             or beyond len into a match, a hash or a sum — `most`, `p < len` —, so n mod 4 = 1 and 3 need nothing the n mod 4 = 2 of the HALF rows
 *                             did not).
 *   deflate   k_zip_deflate / k_zip_deflate_dynamic with a ZipGeom that says "one chunk of n bytes": BFINAL in the last segment only.
 *   crc+scan  k_png_crc       one wave per segment: the CRC register of its output bytes, zero initial value, no conditioning, with x^(8 bytes) mod P beside it.
 *             k_png_scan      one workgroup, workgroup-wide inclusive scans over the segments, 256 at a time, of one monoid element: the offset (a sum), the
 *                             Adler-32 pair of F (a, b and the length: b of a concatenation is b1 + len2 * a1 + b2) and the CRC pair (register, multiplier:
 *                             r(A || B) = r(A) * x^(8 |B|) mod P ^ r(B), a carry-less multiplication mod the CRC polynomial). No loop over the segments runs on one
 *                             lane. The conditioning (initial ~0, final ~), "IDAT", the zlib header and the Adler trailer enter once, at the ends.
 *   emit      k_png_emit      one workgroup per segment copies it behind the IDAT header; the first writes the chunk length, the Adler trailer, the CRC and IEND.
 * The signature, IHDR, the tEXt chunks and the IDAT header are a few dozen bytes the host composes (their CRCs by the same pngCrcByte) and uploads in front.
 * k_png_crc and k_png_scan without the segment sums are crx_debug_crc32: the piece CRC and the combination on bytes of the caller's.
 * Only __shfl_up, __shfl_xor and __syncthreads beside exr_zip.h's helpers: the file compiles unmodified on tests/emu/hipemu.
 */
#pragma once
#include "srgb8.h"

/* ---- CRC-32 (the PNG specification's, polynomial 0xedb88320 bit-reversed) as arithmetic on polynomials over GF(2) mod P: bit 31 of a word is x^0, bit 0 is x^31 ---- */
#define CRX_PNG_POLY 0xedb88320u
#define CRX_PNG_ONE 0x80000000u          /* the polynomial 1 */
__host__ __device__ __forceinline__ uint32_t pngCrcTimesX(uint32_t r) { return (r >> 1) ^ ((r & 1u) ? CRX_PNG_POLY : 0u); }
/* the register after one more byte: no conditioning, that is the caller's */
__host__ __device__ __forceinline__ uint32_t pngCrcByte(uint32_t r, uint32_t byte) {
	r ^= byte;
	for (uint32_t i = 0; i < 8u; ++i) r = pngCrcTimesX(r);
	return r;
}
/* a * b mod P */
__host__ __device__ __forceinline__ uint32_t pngCrcMul(uint32_t a, uint32_t b) {
	uint32_t p = 0u;
	for (uint32_t i = 0; i < 32u; ++i) {
		if (a & (CRX_PNG_ONE >> i)) p ^= b;
		b = pngCrcTimesX(b);
	}
	return p;
}
/* x^(8 bytes) mod P: what `bytes` more bytes multiply a register by (square and multiply, at most 32 rounds) */
__host__ __device__ __forceinline__ uint32_t pngCrcShift(uint32_t bytes) {
	uint32_t r = CRX_PNG_ONE, base = CRX_PNG_ONE >> 8;
	for (; bytes; bytes >>= 1) {
		if (bytes & 1u) r = pngCrcMul(r, base);
		base = pngCrcMul(base, base);
	}
	return r;
}
/* the monoid: the register of a piece taken with a zero initial value, and x^(8 |piece|) */
struct PngCrc { uint32_t reg, mul; };
__host__ __device__ __forceinline__ PngCrc pngCrcJoin(PngCrc l, PngCrc r) { return PngCrc{pngCrcMul(l.reg, r.mul) ^ r.reg, pngCrcMul(l.mul, r.mul)}; }
__host__ __device__ __forceinline__ PngCrc pngCrcOf(const uint8_t *p, uint32_t n) {
	PngCrc c = {0u, pngCrcShift(n)};
	for (uint32_t i = 0; i < n; ++i) c.reg = pngCrcByte(c.reg, p[i]);
	return c;
}

#define CRX_PNG_FIXED_TAIL 20u          /* behind the deflate data: the Adler-32, the IDAT's CRC, IEND */

/* ---- convert ---- */
/* word wi of the 8-bit image [H, W, 3]: bytes 4 wi .. 4 wi + 3 of `count` */
__global__ __launch_bounds__(256) void k_png_convert(const float *fb, uint32_t count, uint32_t *img) {
	const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
	if (4u * (uint64_t)wi >= count) return;
	uint32_t out = 0u;
	for (uint32_t b = 0; b < 4u && 4u * wi + b < count; ++b) out |= (uint32_t)crh::linearToSRGB8(fb[4u * (size_t)wi + b]) << (8u * b);
	img[wi] = out;
}

/* crx_png_pack_display's convert (in k_png_convert's place when a display transform is asked for) and crx_auto_exposure's two kernels */
#include "png_display.h"

/* ---- filter ---- */
/* the PNG specification's predictors for bpp = 3: a is the byte three to the left, b the byte above, c the one above a; bytes off the image count as 0 */
__host__ __device__ __forceinline__ uint32_t pngPredict(uint32_t type, uint32_t a, uint32_t b, uint32_t c) {
	if (type == 1u) return a;
	if (type == 2u) return b;
	if (type == 3u) return (a + b) >> 1;
	if (type == 4u) {
		const int p = (int)a + (int)b - (int)c;
		const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
		return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
	}
	return 0u;
}
/* byte x of row r of the image and its three neighbours */
__device__ __forceinline__ void pngNeighbours(const uint8_t *img, uint32_t rowBytes, uint32_t r, uint32_t x, uint32_t &v, uint32_t &a, uint32_t &b, uint32_t &c) {
	const uint8_t *const row = img + (size_t)r * rowBytes;
	v = row[x];
	a = x >= 3u ? row[x - 3u] : 0u;
	b = r ? (row - rowBytes)[x] : 0u;
	c = r && x >= 3u ? (row - rowBytes)[x - 3u] : 0u;
}

/* One wave per row, four rows a workgroup. filter >= 0: that type on every row. CRX_PNG_FILTER_ADAPTIVE: the type whose filtered bytes have the least sum of
 * min(v, 256 - v), ties to the lowest type. (A lane's sum <= 128 * ceil(3 W / 64) < 2^32; the wave's is taken in two 16-bit halves.) */
__global__ __launch_bounds__(256) void k_png_choose(const uint8_t *img, uint32_t rowBytes, uint32_t height, int filter, uint8_t *types) {
	const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (r >= height) return;          /* (the whole wave) */
	if (filter >= 0) {
		if (lane == 0u) types[r] = (uint8_t)filter;
		return;
	}
	uint32_t sum[5] = {0u, 0u, 0u, 0u, 0u};
	for (uint32_t x = lane; x < rowBytes; x += 64u) {
		uint32_t v, a, b, c;
		pngNeighbours(img, rowBytes, r, x, v, a, b, c);
#pragma unroll
		for (uint32_t t = 0; t < 5u; ++t) {
			const uint32_t f = (v - pngPredict(t, a, b, c)) & 255u;
			sum[t] += zipMin(f, 256u - f);
		}
	}
	uint32_t best = 0u;
	uint64_t least = 0u;
#pragma unroll
	for (uint32_t t = 0; t < 5u; ++t) {
		const uint64_t s = (uint64_t)zipWaveSum(sum[t] & 0xffffu) + ((uint64_t)zipWaveSum(sum[t] >> 16) << 16);
		if (t == 0u || s < least) { least = s; best = t; }
	}
	if (lane == 0u) types[r] = (uint8_t)best;
}

/* F: word wi (bytes 4 wi .. 4 wi + 3 of n); a row is its type byte and rowBytes filtered bytes. The bytes behind n in the last word are zero. */
__global__ __launch_bounds__(256) void k_png_filter(const uint8_t *img, const uint8_t *types, uint32_t rowBytes, uint32_t n, uint32_t *F) {
	const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
	if (4u * (uint64_t)wi >= n) return;
	const uint32_t stride = rowBytes + 1u;
	uint32_t r = 4u * wi / stride, at = 4u * wi - r * stride, out = 0u;
	for (uint32_t k = 0; k < 4u && 4u * wi + k < n; ++k) {
		const uint32_t type = types[r];
		uint32_t byte = type;
		if (at) {
			uint32_t v, a, b, c;
			pngNeighbours(img, rowBytes, r, at - 1u, v, a, b, c);
			byte = (v - pngPredict(type, a, b, c)) & 255u;
		}
		out |= byte << (8u * k);
		if (++at == stride) { at = 0u; ++r; }
	}
	F[wi] = out;
}

/* ---- crc + scan ---- */
/* The CRC pair of n bytes by one wave: a lane takes ceil(n / 64) consecutive bytes, the lanes' pairs join by an inclusive scan; lane 63 holds the piece's. */
__device__ __forceinline__ PngCrc pngWaveCrc(const uint8_t *p, uint32_t n, uint32_t lane) {
	const uint32_t per = (n + 63u) / 64u, lo = zipMin(n, lane * per), hi = zipMin(n, lo + per);
	PngCrc c = pngCrcOf(p + lo, hi - lo);
	for (uint32_t d = 1u; d < 64u; d <<= 1) {
		const PngCrc o = {__shfl_up(c.reg, d), __shfl_up(c.mul, d)};
		if (lane >= d) c = pngCrcJoin(o, c);
	}
	return c;
}

/* One wave per piece. segMeta: piece s is the segMeta[4 s] output bytes of segment s, `pitch` bytes apart (crx_png_pack). Null: piece s is bytes
 * [s * pitch, min(n, (s + 1) * pitch)) (crx_debug_crc32). crcMeta: {register, multiplier} a piece. */
__global__ __launch_bounds__(64) void k_png_crc(const uint8_t *bytes, uint32_t pitch, const uint32_t *segMeta, uint64_t n, uint32_t *crcMeta) {
	const uint64_t begin = (uint64_t)blockIdx.x * pitch;
	const uint32_t len = segMeta ? segMeta[4u * (size_t)blockIdx.x] : (uint32_t)(n - begin < pitch ? n - begin : pitch);
	const PngCrc c = pngWaveCrc(bytes + begin, len, threadIdx.x);
	if (threadIdx.x == 63u) { crcMeta[2u * (size_t)blockIdx.x] = c.reg; crcMeta[2u * (size_t)blockIdx.x + 1u] = c.mul; }
}

/* what the scan carries over the segments: output bytes; bytes of F mod 65521 and the Adler sums of exr_zip.h's segMeta; the CRC pair of the output bytes */
struct PngScan { uint32_t off, len, a, b; PngCrc crc; };
__device__ __forceinline__ PngScan pngScanJoin(const PngScan &l, const PngScan &r) {
	PngScan o;
	o.off = l.off + r.off;
	o.len = (l.len + r.len) % CRX_ADLER;
	o.a = (l.a + r.a) % CRX_ADLER;
	o.b = (uint32_t)(((uint64_t)l.b + (uint64_t)r.len * l.a + r.b) % CRX_ADLER);
	o.crc = pngCrcJoin(l.crc, r.crc);
	return o;
}
__device__ __forceinline__ PngScan pngScanUp(const PngScan &e, uint32_t d) {
	PngScan o;
	o.off = __shfl_up(e.off, d); o.len = __shfl_up(e.len, d); o.a = __shfl_up(e.a, d); o.b = __shfl_up(e.b, d);
	o.crc.reg = __shfl_up(e.crc.reg, d); o.crc.mul = __shfl_up(e.crc.mul, d);
	return o;
}

/* One workgroup of 256. `count` pieces, 256 at a time: an inclusive scan within each wave, the waves' totals through LDS, the tiles before as a carry every lane
 * keeps. segMeta (crx_png_pack: n bytes of F in segments of CRX_SEG) or null (crx_debug_crc32: the CRC alone); segOff: where a segment's bytes start in the deflate
 * data. info: {deflate bytes, Adler-32 of F, the CRC-32, 0} — the CRC of "IDAT", 78 01, the pieces and the Adler trailer with segMeta, of the pieces without. */
__global__ __launch_bounds__(256) void k_png_scan(const uint32_t *segMeta, const uint32_t *crcMeta, uint32_t count, uint32_t n, uint32_t *segOff, uint32_t *info) {
	__shared__ uint32_t sWave[4][6];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const PngScan none = {0u, 0u, 0u, 0u, {0u, CRX_PNG_ONE}};
	PngScan carry = none;
	for (uint32_t base = 0u; base < count; base += 256u) {
		const uint32_t s = base + threadIdx.x;
		PngScan e = none;
		if (s < count) {
			e.crc.reg = crcMeta[2u * (size_t)s]; e.crc.mul = crcMeta[2u * (size_t)s + 1u];
			if (segMeta) {
				const uint32_t *const meta = segMeta + 4u * (size_t)s;
				e.off = meta[0]; e.len = zipMin(CRX_SEG, n - s * CRX_SEG) % CRX_ADLER; e.a = meta[1]; e.b = meta[2];
			}
		}
		const uint32_t own = e.off;
		for (uint32_t d = 1u; d < 64u; d <<= 1) {
			const PngScan o = pngScanUp(e, d);
			if (lane >= d) e = pngScanJoin(o, e);
		}
		if (lane == 63u) { sWave[wave][0] = e.off; sWave[wave][1] = e.len; sWave[wave][2] = e.a; sWave[wave][3] = e.b; sWave[wave][4] = e.crc.reg; sWave[wave][5] = e.crc.mul; }
		__syncthreads();
		PngScan before = carry;
		for (uint32_t w = 0u; w < 4u; ++w) {
			const PngScan t = {sWave[w][0], sWave[w][1], sWave[w][2], sWave[w][3], {sWave[w][4], sWave[w][5]}};
			if (w == wave) e = pngScanJoin(before, e);
			before = pngScanJoin(before, t);
		}
		if (segOff && s < count) segOff[s] = e.off - own;
		carry = before;
		__syncthreads();
	}
	if (threadIdx.x != 0u) return;
	const uint32_t adler = ((carry.b + carry.len) % CRX_ADLER) << 16 | (1u + carry.a) % CRX_ADLER;          /* the initial a = 1 is in every byte's b */
	PngCrc c = {0xffffffffu, CRX_PNG_ONE};
	if (segMeta) {
		const uint8_t head[6] = {'I', 'D', 'A', 'T', 0x78, 0x01}, tail[4] = {(uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
		c = pngCrcJoin(pngCrcJoin(pngCrcJoin(c, pngCrcOf(head, 6u)), carry.crc), pngCrcOf(tail, 4u));
	} else c = pngCrcJoin(c, carry.crc);
	info[0] = carry.off; info[1] = adler; info[2] = ~c.reg; info[3] = 0u;
}

/* ---- emit ---- */
__device__ __forceinline__ void pngStore4(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

/* One workgroup per segment: its bytes to their place in the file. `at`: where the IDAT chunk starts in `out` — its length, "IDAT", 78 01, then the deflate data;
 * everything in front of the length, "IDAT" and 78 01 are there already. */
__global__ __launch_bounds__(256) void k_png_emit(const uint32_t *segOut, const uint32_t *segMeta, const uint32_t *segOff, const uint32_t *info, uint8_t *out, uint32_t at) {
	uint8_t *const data = out + at + 10u;
	const uint32_t bytes = segMeta[4u * (size_t)blockIdx.x];
	const uint8_t *const from = (const uint8_t *)(segOut + (size_t)blockIdx.x * (CRX_SEG_OUT / 4u));
	uint8_t *const to = data + segOff[blockIdx.x];
	for (uint32_t i = threadIdx.x; i < bytes; i += 256u) to[i] = from[i];
	if (blockIdx.x == 0u && threadIdx.x == 0u) {
		const uint32_t size = info[0];
		pngStore4(out + at, 2u + size + 4u);
		pngStore4(data + size, info[1]);
		pngStore4(data + size + 4u, info[2]);
		const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
		for (uint32_t i = 0; i < 12u; ++i) data[size + 8u + i] = iend[i];
	}
}
