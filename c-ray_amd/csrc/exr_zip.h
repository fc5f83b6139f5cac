/*
 * exr_zip.h — the kernels of crx_pack_zip and crx_pack (include/cray_hip_exr.h): the chunks of a ZIP / ZIPS compressed scanline OpenEXR file, deflated on the device,
 * with FLOAT or — crx_pack — per channel HALF pixels. Part of libcray_hip_exr.so (exr_zip.hip); nothing of libcray_hip.so includes this file.
 *
 * Four launches on one stream, ordered by launch order alone — no workgroup waits for another, every loop's trip count follows from CRX_SEG or the chunk size:
 *   k_zip_transform  gather + byte split + predictor in one pass: a lane makes four consecutive bytes of T' from the (at most three) raw words they come from,
 *                    read straight from the channel sources; stores are coalesced words. No raw copy of a chunk exists.
 *   k_zip_deflate    one wave per segment of CRX_SEG bytes of T', staged in LDS, in 64 steps: lane l of step i stands at position 64 i + l. Every step enters its
 *                    positions' 3-byte hashes in a table of last positions — it reads the table, a barrier, then atomicMax: what a position finds is the last
 *                    occurrence in an EARLIER step, whatever the lane timing. A step that a match taken earlier covers whole is done with that. Otherwise its
 *                    positions from the next token start on try the distances 1 .. 4 (after the split, constant words are period-1 or period-2 byte patterns)
 *                    and the table's candidate; lengths are compared four bytes at a time, up to 258, never past the segment. The greedy parse (longest match
 *                    of at least 3 at a token start, else a literal) runs through the step by __shfl of the lanes' advances, at most 64 rounds; the tokens'
 *                    fixed-Huffman codes go into an LDS bit buffer behind an inclusive scan of their bit lengths, by atomicOr. Every segment but a chunk's last
 *                    ends with an empty stored block (00 00 ff ff behind a byte boundary), so segments concatenate as bytes; BFINAL is set in the chunk's last
 *                    block only. The segment's Adler-32 sums are taken alongside.
 *   k_zip_scan       one workgroup: per chunk the offsets of its segments, the combined Adler-32 and the choice stream / raw (raw where the stream is not
 *                    shorter than n); then the chunks' positions in the output, their byte counts and the total.
 *   k_zip_emit       one workgroup per segment copies it behind the chunk's 8-byte header and the zlib header — or, in a raw chunk, gathers that stretch of
 *                    raw bytes from the sources; the first writes the headers and the Adler-32 trailer.
 * A call whose channels are all FLOAT runs exactly these. A call with a HALF channel (crx_pack) runs k_zip_transform_mixed and k_zip_emit_mixed in their places —
 * the MIXED == true instantiations of the bodies (zipTransform, zipEmit) whose MIXED == false instantiations the plain kernels are —:
 * a row is no longer nch * width words but one plane of 2- or 4-byte pixels per channel, so byte i of a chunk is found as line i / rowBytes, the channel whose
 * stretch of the row holds the rest (a binary search in the prefix table of the channels' byte offsets, at most 65 words, in LDS), pixel and byte within the
 * pixel; a lane still makes four consecutive bytes of T' and stores one word. n is even but not always a multiple of 4: the T' pitch is whole words, the two
 * bytes behind an n = 2 (mod 4) are stored as zero, k_zip_deflate takes no position at or beyond len into a match or a sum (`most`, `p < len`), and the raw
 * gather ends in a 2-byte store. Compression 0 (crx_pack) launches only k_zip_scan, which then marks every chunk raw, and the emit.
 * Under crx_set_codes(CRX_CODES_DYNAMIC) k_zip_deflate_dynamic runs in k_zip_deflate's place: zipDeflate<true> where that is zipDeflate<false>. The parse exists
 * once (zipParse) and runs twice there: the first run counts the tokens' symbols into LDS histograms (286 lit/len, 30 distance words, atomicAdd), zipChooseCodes
 * builds a length-limited Huffman code for each (zipCodeLengths: a ranking sort, a two-queue merge by one lane, zlib's overflow repair), run-length codes the
 * lengths, builds the code-length code, compares the block's bits under these codes, header included, with its bits under the fixed codes, and leaves in LDS the
 * code tables the second run emits under — the dynamic codes behind their header, or, on a tie or a loss, the fixed codes themselves. Nothing per position is kept
 * between the runs; the bit buffer, not yet written, is the scratch of the construction. k_zip_code_lengths (crx_debug_code_lengths) runs zipCodeLengths alone.
 * Only __ballot, __popcll, __shfl, __shfl_up, __shfl_xor, __syncthreads and atomicAdd / atomicMax / atomicOr on 32-bit LDS words: the file compiles unmodified on
 * tests/emu/hipemu.
 */
#pragma once

/* binary32 -> binary16, the rule of include/cray_hip_exr.h, in integer arithmetic: the same bits on the device, on the emulation and in tests/emu/half_check.cpp
 * (which defines CRX_ZIP_CONVERSION_ONLY and takes this function alone). Round to nearest, ties to even; gradual underflow; |x| < 2^-25 and the tie 2^-25 to +-0;
 * what rounds to 2^16 or more (|x| >= 65520) to +-infinity; a NaN keeps its top ten mantissa bits, bit 0 set if those are all zero. */
__host__ __device__ __forceinline__ uint32_t zipHalfBits(uint32_t w) {
	const uint32_t sign = (w >> 16) & 0x8000u, a = w & 0x7fffffffu;
	if (a > 0x7f800000u) { const uint32_t m = (a >> 13) & 0x3ffu; return sign | 0x7c00u | m | (m == 0u ? 1u : 0u); }
	if (a >= 0x477ff000u) return sign | 0x7c00u;          /* infinity, and what rounds to 2^16 or more */
	if (a >= 0x38800000u) {                               /* a normal half: exponent rebiased by 112, rounded at bit 13 (a carry runs into the exponent) */
		const uint32_t v = a - 0x38000000u;
		return sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13);
	}
	if (a < 0x33000000u) return sign;                     /* below 2^-25 */
	const uint32_t shift = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u;          /* 14 .. 24: units of 2^-24 */
	const uint32_t r = m >> shift, rest = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
	return sign | (r + (rest > tie || (rest == tie && (r & 1u)) ? 1u : 0u));
}

#ifndef CRX_ZIP_CONVERSION_ONLY
#define CRX_SEG 4096u                 /* bytes of T' per segment (a multiple of 256) */
#define CRX_SEG_OUT 4640u             /* bytes a segment's output can take: 3 + 9 * CRX_SEG + 7 + 3 bits, padded to a byte, + 4: 4614, rounded up to a multiple of 32.
                                       * Derived for the fixed codes; it holds for CRX_CODES_DYNAMIC as it is: a dynamic block is written only where it has fewer bits */
#define CRX_HASH_BITS 11
#define CRX_MAX_MATCH 258u
#define CRX_ADLER 65521u

struct ZipChan {
	const uint32_t *src;          /* [H, W, stride] words */
	const uint32_t *map;          /* device copy of the map, or null */
	uint32_t stride, component, mapCount, half;          /* half: stored as binary16 (never with a map) */
};
struct ZipArgs { ZipChan ch[CRH_PACK_MAX_CHANNELS]; };
struct ZipRow { uint32_t off[CRH_PACK_MAX_CHANNELS + 1u]; };          /* where channel c's plane starts in a stored row, in bytes; off[nch] = rowBytes */
struct ZipGeom {
	uint32_t nch, width, firstRow, rowCount;          /* rowCount rows from stored row firstRow */
	uint32_t lpc, nchunks;                            /* lines per chunk, chunks of this call */
	uint32_t fullBytes;                               /* rowBytes * lpc: the raw bytes of a full chunk */
	uint32_t segsPerChunk;                            /* ceil(fullBytes / CRX_SEG) */
	uint32_t rowBytes;                                /* width * the sum of the channels' pixel sizes: 4 * nch * width where all are FLOAT */
	uint32_t pitch;                                   /* words a chunk in the T' buffer: ceil(fullBytes / 4) */
	uint32_t allRaw;                                  /* compression 0: k_zip_scan marks every chunk raw, nothing was deflated */
};

__host__ __device__ __forceinline__ uint32_t zipMin(uint32_t a, uint32_t b) { return a < b ? a : b; }
/* raw bytes of chunk k of the call (the last one of the image may be short) */
__host__ __device__ __forceinline__ uint32_t zipChunkBytes(const ZipGeom &G, uint32_t k) { return G.rowBytes * zipMin(G.lpc, G.rowCount - k * G.lpc); }

/* the word a mapped channel stores for the source word w (exr_pack.h's rule: converted only once it is known to lie in [0, mapCount)) */
__device__ __forceinline__ uint32_t zipMapped(const ZipChan &k, uint32_t w) {
	const float v = __builtin_bit_cast(float, w);
	uint32_t out = 0u;
	if (v >= 0.0f && v < (float)k.mapCount) {
		const uint32_t u = (uint32_t)v;
		if ((float)u == v) out = k.map[u];
	}
	return out;
}

/* word wi of chunk k's raw bytes: [line][channel][x] */
__device__ __forceinline__ uint32_t zipRawWord(const ZipArgs &A, const ZipGeom &G, uint32_t k, uint32_t wi) {
	const uint32_t perRow = G.nch * G.width;
	const uint32_t line = wi / perRow, rem = wi - line * perRow;
	const uint32_t c = rem / G.width, x = rem - c * G.width;
	const uint32_t y = G.firstRow + k * G.lpc + line;
	const ZipChan &ch = A.ch[c];
	uint32_t w = ch.src[((size_t)y * G.width + x) * ch.stride + ch.component];
	if (ch.map) w = zipMapped(ch, w);
	return w;
}

/* ---- mixed HALF / FLOAT rows: what k_zip_transform_mixed and k_zip_emit_mixed read their bytes through ---- */
/* the element last fetched: bytes [lo, hi) of the chunk are the little-endian bytes of v; it lies in the plane [planeLo, planeHi) of channel c on stored row y */
struct ZipHeld { uint32_t lo, hi, v, planeLo, planeHi, c, y; };

/* byte i of chunk k's raw bytes; off: the prefix table in LDS. Consecutive calls mostly stay in one plane: only leaving it costs the division and the search. */
__device__ __forceinline__ uint32_t zipMixedByte(const ZipArgs &A, const ZipGeom &G, const uint32_t *off, uint32_t k, uint32_t i, ZipHeld &h) {
	if (i < h.lo || i >= h.hi) {
		if (i < h.planeLo || i >= h.planeHi) {
			const uint32_t line = i / G.rowBytes, rest = i - line * G.rowBytes;
			uint32_t c = 0u, end = G.nch;          /* off[c] <= rest < off[end] */
			while (end - c > 1u) {
				const uint32_t mid = (c + end) >> 1;
				if (off[mid] <= rest) c = mid; else end = mid;
			}
			h.c = c; h.y = G.firstRow + k * G.lpc + line;
			h.planeLo = line * G.rowBytes + off[c]; h.planeHi = line * G.rowBytes + off[c + 1u];
		}
		const ZipChan &ch = A.ch[h.c];
		const uint32_t within = i - h.planeLo, x = ch.half ? within >> 1 : within >> 2;
		uint32_t w = ch.src[((size_t)h.y * G.width + x) * ch.stride + ch.component];
		if (ch.map) w = zipMapped(ch, w);
		if (ch.half) { h.v = zipHalfBits(w); h.lo = h.planeLo + 2u * x; h.hi = h.lo + 2u; }
		else { h.v = w; h.lo = h.planeLo + 4u * x; h.hi = h.lo + 4u; }
	}
	return (h.v >> (8u * (i - h.lo))) & 255u;
}

/* T': word wi of every chunk (bytes 4 wi .. 4 wi + 3), blocksPerChunk workgroups of 256 lanes a chunk. MIXED: rows with HALF channels (off: their prefix table
 * in LDS) — the same four bytes of T' a lane, from up to five elements instead of three words; n is even, not always a multiple of 4, and the bytes behind n in a
 * chunk's last word are zero */
template <bool MIXED>
__device__ __forceinline__ void zipTransform(const ZipArgs &A, const ZipGeom &G, const uint32_t *off, uint32_t blocksPerChunk, uint32_t *T) {
	const uint32_t k = blockIdx.x / blocksPerChunk, wi = (blockIdx.x - k * blocksPerChunk) * 256u + threadIdx.x;
	const uint32_t n = zipChunkBytes(G, k);          /* !MIXED: a multiple of 4, (n + 1) / 2 == n / 2 */
	if (4u * wi >= n) return;
	const uint32_t half = n / 2u;
	uint32_t heldAt = 0xffffffffu, held = 0u;          /* !MIXED: the raw word last fetched: consecutive bytes of T come from the same or the next one */
	ZipHeld h = {0u, 0u, 0u, 0u, 0u, 0u, 0u};          /* MIXED: the element last fetched */
	uint32_t t[5];
	for (uint32_t b = 0; b < 5u; ++b) {                /* T[4 wi - 1] .. T[4 wi + 3] */
		const uint32_t j = 4u * wi + b - 1u;
		if ((wi == 0u && b == 0u) || (MIXED && j >= n)) { t[b] = 0u; continue; }
		const uint32_t i = j < half ? 2u * j : 2u * (j - half) + 1u;
		if (MIXED) t[b] = zipMixedByte(A, G, off, k, i, h);
		else {
			if ((i >> 2) != heldAt) { heldAt = i >> 2; held = zipRawWord(A, G, k, heldAt); }
			t[b] = (held >> (8u * (i & 3u))) & 255u;
		}
	}
	uint32_t out = 0u;
	for (uint32_t b = 0; b < 4u; ++b) {
		if (MIXED && 4u * wi + b >= n) break;
		out |= ((wi == 0u && b == 0u ? t[1] : t[b + 1] - t[b] + 128u) & 255u) << (8u * b);
	}
	T[(size_t)k * G.pitch + wi] = out;
}

__global__ __launch_bounds__(256) void k_zip_transform(const ZipArgs A, const ZipGeom G, uint32_t blocksPerChunk, uint32_t *T) {
	zipTransform<false>(A, G, nullptr, blocksPerChunk, T);
}

__global__ __launch_bounds__(256) void k_zip_transform_mixed(const ZipArgs A, const ZipRow R, const ZipGeom G, uint32_t blocksPerChunk, uint32_t *T) {
	__shared__ uint32_t sOff[CRH_PACK_MAX_CHANNELS + 1u];
	if (threadIdx.x <= G.nch) sOff[threadIdx.x] = R.off[threadIdx.x];
	__syncthreads();
	zipTransform<true>(A, G, sOff, blocksPerChunk, T);
}

/* ---- fixed Huffman codes (RFC 1951, 3.2.6), packed from bit 0: Huffman codes enter most significant bit first, extra bits least significant first ---- */
__host__ __device__ __forceinline__ uint32_t zipRev(uint32_t v, uint32_t bits) {
	uint32_t r = 0u;
	for (uint32_t i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1u - i);
	return r;
}
__host__ __device__ __forceinline__ uint32_t zipLog2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }          /* v >= 1 */
__host__ __device__ __forceinline__ void zipLiteral(uint32_t byte, uint64_t &code, uint32_t &bits) {
	if (byte < 144u) { code = zipRev(0x30u + byte, 8u); bits = 8u; }
	else { code = zipRev(0x190u + byte - 144u, 9u); bits = 9u; }
}
/* the symbols of a match (RFC 1951, 3.2.5), whatever codes they get: length 3 .. 258 -> lit/len symbol 257 .. 285 and e extra bits x; distance 1 .. 32768 ->
 * distance symbol 0 .. 29 and de extra bits dx */
__host__ __device__ __forceinline__ void zipMatchSymbols(uint32_t length, uint32_t distance, uint32_t &sym, uint32_t &e, uint32_t &x, uint32_t &dc, uint32_t &de, uint32_t &dx) {
	const uint32_t l = length - 3u;
	e = 0u; x = 0u;
	if (length == 258u) sym = 285u;
	else if (l < 8u) sym = 257u + l;
	else { e = zipLog2(l) - 2u; sym = 261u + 4u * e + ((l >> e) - 4u); x = l & ((1u << e) - 1u); }
	const uint32_t dd = distance - 1u;
	dc = dd; de = 0u; dx = 0u;
	if (dd >= 4u) { de = zipLog2(dd) - 1u; dc = 2u * de + 2u + ((dd >> de) & 1u); dx = dd & ((1u << de) - 1u); }
}
/* the fixed code of a lit/len symbol 256 .. 287: 7 or 8 bits */
__host__ __device__ __forceinline__ void zipFixedLength(uint32_t sym, uint32_t &code, uint32_t &bits) {
	if (sym < 280u) { code = zipRev(sym - 256u, 7u); bits = 7u; }
	else { code = zipRev(0xc0u + sym - 280u, 8u); bits = 8u; }
}
/* length 3 .. 258, distance 1 .. 32768: at most 8 + 5 + 5 + 13 = 31 bits */
__host__ __device__ __forceinline__ void zipMatch(uint32_t length, uint32_t distance, uint64_t &code, uint32_t &bits) {
	uint32_t sym, e, x, dc, de, dx, c, n;
	zipMatchSymbols(length, distance, sym, e, x, dc, de, dx);
	zipFixedLength(sym, c, n);
	code = c;
	code |= (uint64_t)x << n; n += e;
	code |= (uint64_t)zipRev(dc, 5u) << n; n += 5u;
	code |= (uint64_t)dx << n; n += de;
	bits = n;
}

/* four bytes of the staged segment from byte position p, any alignment (the words behind the segment are zero) */
__device__ __forceinline__ uint32_t zipLoad4(const uint32_t *data, uint32_t p) {
	const uint32_t w = p >> 2, s = 8u * (p & 3u);
	const uint32_t lo = data[w];
	return s ? (lo >> s) | (data[w + 1u] << (32u - s)) : lo;
}
/* how many bytes from p equal those `distance` before them, at most `most` (<= CRX_MAX_MATCH: at most 65 rounds) */
__device__ __forceinline__ uint32_t zipMatchLength(const uint32_t *data, uint32_t p, uint32_t distance, uint32_t most) {
	uint32_t l = 0u;
	while (l < most) {
		const uint32_t x = zipLoad4(data, p + l) ^ zipLoad4(data, p - distance + l);
		if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
		l += 4u;
	}
	return zipMin(l, most);
}

/* `bits` bits of `code` per lane into the LDS bit buffer, each lane's behind those of the lanes below, from bit `at` (wave-uniform): the new `at`.
 * WIDE: a code of more than 33 bits (a match under a dynamic code: up to 15 + 5 + 15 + 13 = 48) can reach a third word */
template <bool WIDE>
__device__ __forceinline__ uint32_t zipPut(uint32_t *sBits, uint32_t at, uint32_t lane, uint64_t code, uint32_t bits) {
	uint32_t sum = bits;
	for (uint32_t d = 1u; d < 64u; d <<= 1) {
		const uint32_t below = __shfl_up(sum, d);
		if (lane >= d) sum += below;
	}
	if (bits) {
		const uint32_t off = at + sum - bits, s = off & 31u;
		const uint64_t v = (WIDE ? code & 0xffffffffu : code) << s;
		atomicOr(&sBits[off >> 5], (uint32_t)v);
		if (WIDE) {
			const uint64_t hi = (code >> 32) << s;
			const uint32_t second = (uint32_t)(v >> 32) | (uint32_t)hi;
			if (second) atomicOr(&sBits[(off >> 5) + 1u], second);
			if (hi >> 32) atomicOr(&sBits[(off >> 5) + 2u], (uint32_t)(hi >> 32));
		} else if (v >> 32) atomicOr(&sBits[(off >> 5) + 1u], (uint32_t)(v >> 32));
	}
	return at + __shfl(sum, 63);
}

/* what a run of the parse does with its tokens */
enum { ZIP_FIXED = 0,          /* emits them under the fixed codes */
       ZIP_COUNT = 1,          /* counts their symbols: lit[286] and dist[30] are histograms */
       ZIP_TABLE = 2 };        /* emits them under the codes in lit[288] and dist[32]: a word is the code, reversed, << 4 | its length */

/* THE parse of a staged segment, the 64 steps of the header comment: sHash must be zero. Deterministic: every run over the same bytes makes the same tokens. Returns
 * the bits written so far (from `at`); the emitting runs take the Adler-32 sums alongside. */
template <int WHAT>
__device__ __forceinline__ uint32_t zipParse(const uint32_t *sData, uint32_t *sHash, uint32_t *sBits, uint32_t *lit, uint32_t *dist, uint32_t len, uint32_t lane, uint32_t at,
                                             uint32_t &sumA, uint32_t &sumB) {
	uint32_t next = 0u;                     /* where the next token starts: the greedy parse, wave-uniform */
	for (uint32_t step = 0; step < CRX_SEG / 64u; ++step) {
		const uint32_t base = 64u * step, p = base + lane;
		const uint32_t most = p < len ? zipMin(CRX_MAX_MATCH, len - p) : 0u;
		uint32_t h = 0u, seen = 0u, byte = 0u;
		if (p < len) {
			const uint32_t four = zipLoad4(sData, p);
			byte = four & 255u;
			if (WHAT != ZIP_COUNT) { sumA += byte; sumB += (len - p) * byte; }
			if (most >= 3u) { h = ((four & 0xffffffu) * 2654435761u) >> (32u - CRX_HASH_BITS); seen = sHash[h]; }
		}
		__syncthreads();
		if (most >= 3u) atomicMax(&sHash[h], p + 1u);
		__syncthreads();
		if (next >= base + 64u || base >= len) continue;          /* a match taken earlier covers the step, or the segment has ended: nothing starts here */

		/* the matches of the positions a token can start at */
		uint32_t best = 0u, bestDistance = 0u;
		if (most >= 3u && p >= next) {
			for (uint32_t d = 1u; d <= 4u && d <= p && best < most; ++d) {
				const uint32_t l = zipMatchLength(sData, p, d, most);
				if (l > best) { best = l; bestDistance = d; }
			}
			if (seen && best < most) {
				const uint32_t d = p + 1u - seen, l = zipMatchLength(sData, p, d, most);
				if (l > best) { best = l; bestDistance = d; }
			}
		}
		if (best < 3u) best = 0u;
		/* the greedy parse through the step: at most 64 rounds */
		const uint32_t advance = best ? best : 1u, end = zipMin(base + 64u, len);
		bool token = false;
		while (next < end) {
			const uint32_t a = __shfl(advance, (int)(next - base));
			if (p == next) token = true;
			next += a;
		}
		if (WHAT == ZIP_COUNT) {
			if (token && best) {
				uint32_t sym, e, x, dc, de, dx;
				zipMatchSymbols(best, bestDistance, sym, e, x, dc, de, dx);
				atomicAdd(&lit[sym], 1u);
				atomicAdd(&dist[dc], 1u);
			} else if (token) atomicAdd(&lit[byte], 1u);
			continue;
		}
		/* the tokens' codes, each behind those of the lanes below */
		uint64_t code = 0u;
		uint32_t bits = 0u;
		if (token && WHAT == ZIP_FIXED) {
			if (best) zipMatch(best, bestDistance, code, bits);
			else zipLiteral(byte, code, bits);
		} else if (token && best) {
			uint32_t sym, e, x, dc, de, dx;
			zipMatchSymbols(best, bestDistance, sym, e, x, dc, de, dx);
			const uint32_t l = lit[sym], d = dist[dc];
			code = l >> 4; bits = l & 15u;
			code |= (uint64_t)x << bits; bits += e;
			code |= (uint64_t)(d >> 4) << bits; bits += d & 15u;
			code |= (uint64_t)dx << bits; bits += de;
		} else if (token) { code = lit[byte] >> 4; bits = lit[byte] & 15u; }
		at = zipPut<WHAT == ZIP_TABLE>(sBits, at, lane, code, bits);
	}
	return at;
}

/* ---- dynamic Huffman codes (RFC 1951, 3.2.7) ---- */
#define CRX_LIT 286u                  /* lit/len symbols a block can use */
#define CRX_DIST 30u
#define CRX_CL 19u                    /* the code-length alphabet */
#define CRX_MAX_SYMBOLS 288u          /* the largest alphabet zipCodeLengths takes */
#define CRX_FREQ_LIMIT (1u << 23)     /* a histogram's sum stays below this: a sort key is freq << 9 | symbol, a tree's weight one word */
#define CRX_LEN_SCRATCH(symbols) (4u * (symbols) + 16u)          /* words of LDS zipCodeLengths works in */
static_assert(CRX_LEN_SCRATCH(CRX_LIT) <= CRX_SEG_OUT / 4u, "the bit buffer, not yet written, is the scratch of the code construction");

__device__ __forceinline__ uint32_t zipWaveSum(uint32_t v) {
	for (uint32_t d = 32u; d >= 1u; d >>= 1) v += __shfl_xor(v, (int)d);
	return v;
}
__device__ __forceinline__ uint32_t zipWaveMax(uint32_t v) {
	for (uint32_t d = 32u; d >= 1u; d >>= 1) { const uint32_t o = __shfl_xor(v, (int)d); v = o > v ? o : v; }
	return v;
}
__host__ __device__ __forceinline__ uint32_t zipFixedLitBits(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

/* The lengths of a prefix code for the histogram tab[0 .. symbols) in LDS, none longer than `limit` (7 or 15), written over the histogram; the whole wave calls it.
 * A zero count gets length 0. One used symbol gets length 1 and that is all (an incomplete code: inflate allows it for a lit/len or distance code, the caller
 * mends a code-length code). Two or more: a complete code, Kraft sum exactly 1 —
 *   the used symbols sorted by (count, symbol) by ranking (every lane counts the keys below its own);
 *   Huffman's tree by one lane, two queues — the sorted leaves and the nodes made so far, which come out in non-decreasing weight —, a leaf before a node of equal
 *   weight: the tree of least depth among the optimal ones, at most symbols - 1 merges; depths from the root down;
 *   the number of leaves per depth, depths beyond the limit counted at the limit; if that oversubscribes the code, zlib's repair on the counts: the deepest leaf
 *   above the limit becomes a node over itself and a leaf taken from the limit, one unit of 2^-limit less a round (should the limit's count run out first, a
 *   leaf is lengthened instead and what that overshoots is given back by shortening the deepest leaves that fit);
 *   lengths by rank: the rarest symbols get the longest codes. With no repair that is Huffman's cost exactly.
 * scratch: CRX_LEN_SCRATCH(symbols) words of LDS; its last 16 hold, on return, how many symbols have each length. Returns this lane's share of sum count * length. */
__device__ __forceinline__ uint32_t zipCodeLengths(uint32_t *tab, uint32_t symbols, uint32_t limit, uint32_t *scratch, uint32_t lane) {
	uint32_t *const S = scratch, *const W = S + symbols, *const PL = W + symbols, *const PI = PL + symbols, *const CNT = PI + symbols;
	uint32_t n = 0u;
	for (uint32_t base = 0u; base < symbols; base += 64u) n += (uint32_t)__popcll((unsigned long long)__ballot(base + lane < symbols && tab[base + lane] != 0u));
	if (lane < 16u) CNT[lane] = 0u;
	for (uint32_t s = lane; s < symbols; s += 64u) {
		const uint32_t f = tab[s];
		if (!f) continue;
		const uint32_t key = f << 9 | s;
		uint32_t r = 0u;
		for (uint32_t j = 0u; j < symbols; ++j) {
			const uint32_t fj = tab[j];
			if (fj && (fj << 9 | j) < key) ++r;
		}
		S[r] = key;
	}
	__syncthreads();
	if (n <= 1u) {
		uint32_t cost = 0u;
		if (n == 1u && lane == 0u) { tab[S[0] & 511u] = 1u; CNT[1] = 1u; cost = S[0] >> 9; }
		__syncthreads();
		return cost;
	}
	if (lane == 0u) {
		uint32_t i = 0u, j = 0u, leaf = S[0] >> 9, node = 0u;          /* the queues' heads and their weights */
		for (uint32_t m = 0u; m + 1u < n; ++m) {
			uint32_t w = 0u;
			for (uint32_t k = 0u; k < 2u; ++k) {
				if (i < n && (j >= m || leaf <= node)) { w += leaf; PL[i] = m; ++i; leaf = i < n ? S[i] >> 9 : 0u; }
				else { w += node; PI[j] = m; ++j; node = j < m ? W[j] : 0u; }
			}
			W[m] = w;
			if (j == m) node = w;
		}
		W[n - 2u] = 0u;          /* from here on W is a node's depth */
		for (uint32_t k = n - 2u; k-- > 0u;) W[k] = W[PI[k]] + 1u;
	}
	__syncthreads();
	for (uint32_t i = lane; i < n; i += 64u) atomicAdd(&CNT[zipMin(W[PL[i]] + 1u, limit)], 1u);
	__syncthreads();
	if (lane == 0u) {
		const uint32_t full = 1u << limit;
		uint32_t K = 0u;          /* the Kraft sum in units of 2^-limit (<= 288 << 14) */
		for (uint32_t b = 1u; b <= limit; ++b) K += CNT[b] << (limit - b);
		while (K > full) {
			uint32_t b = limit - 1u;
			while (b > 1u && CNT[b] == 0u) --b;
			if (CNT[limit]) { CNT[b] -= 1u; CNT[b + 1u] += 2u; CNT[limit] -= 1u; K -= 1u; }
			else { CNT[b] -= 1u; CNT[b + 1u] += 1u; K -= 1u << (limit - b - 1u); }
		}
		while (K < full) {
			uint32_t b = limit;
			while (b > 2u && (CNT[b] == 0u || (1u << (limit - b)) > full - K)) --b;
			CNT[b] -= 1u; CNT[b - 1u] += 1u; K += 1u << (limit - b);
		}
	}
	__syncthreads();
	uint32_t cost = 0u;
	for (uint32_t i = lane; i < n; i += 64u) {
		uint32_t b = limit, upTo = CNT[limit];
		while (i >= upTo && b > 1u) { --b; upTo += CNT[b]; }
		const uint32_t key = S[i];
		tab[key & 511u] = b;
		cost += (key >> 9) * b;
	}
	__syncthreads();
	return cost;
}

/* Canonical codes (RFC 1951, 3.2.2) for the lengths in tab[0 .. symbols), none above LIMIT; count[b]: how many symbols have length b. A used symbol's word
 * becomes its code, reversed (codes enter the stream most significant bit first), << 4 | its length. The whole wave calls it. */
template <uint32_t LIMIT>
__device__ __forceinline__ void zipAssignCodes(uint32_t *tab, uint32_t symbols, const uint32_t *count, uint32_t lane) {
	uint32_t nextCode[LIMIT + 1u], code = 0u;
	nextCode[0] = 0u;
#pragma unroll
	for (uint32_t b = 1u; b <= LIMIT; ++b) { code = (code + count[b - 1u]) << 1; nextCode[b] = code; }
	const uint64_t below = (1ull << lane) - 1ull;
	for (uint32_t base = 0u; base < symbols; base += 64u) {
		const uint32_t s = base + lane, l = s < symbols ? tab[s] : 0u;
		uint32_t mine = 0u;
#pragma unroll
		for (uint32_t b = 1u; b <= LIMIT; ++b) {
			const uint64_t m = (uint64_t)__ballot(l == b);
			if (l == b) mine = nextCode[b] + (uint32_t)__popcll((unsigned long long)(m & below));
			nextCode[b] += (uint32_t)__popcll((unsigned long long)m);
		}
		if (l) tab[s] = zipRev(mine, l) << 4 | l;
	}
	__syncthreads();
}

/* entry j of the order in which a dynamic block sends the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits an entry */
__host__ __device__ __forceinline__ uint32_t zipClOrder(uint32_t j) {
	const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
	const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
	return (uint32_t)((j < 12u ? lo >> (5u * j) : hi >> (5u * (j - 12u))) & 31u);
}

/* Between the two runs of the parse of a dynamic call. In: the segment's histograms sLit[288] and sDist[32] (the end of block counted). Out: the code tables
 * ZIP_TABLE emits under, and the block's header in the zeroed bit buffer; returns the bits written. The lit/len and distance codes are built from the histograms,
 * their lengths run-length coded as one sequence (position by position: a run of zeros goes in blocks of 138 — symbol 18 for 11 or more, 17 for 3 .. 10, zeros
 * as they are below that —, another value once and then in blocks of 6 — symbol 16 for 3 or more), the code-length code built from those tokens; then the block's
 * bits under these codes, header included, against its bits under the fixed codes, the extra bits of lengths and distances being the same on both sides. Fewer
 * bits: the dynamic header is written and the tables hold the dynamic codes. Otherwise — a tie goes to fixed — the tables hold the fixed codes: ZIP_TABLE then
 * writes what ZIP_FIXED writes. sBits is the scratch of all this and is zeroed at the end, as is sHash. */
__device__ __forceinline__ uint32_t zipChooseCodes(uint32_t *sLit, uint32_t *sDist, uint32_t *sCl, uint32_t *sBits, uint32_t *sHash, bool last, uint32_t lane) {
	uint32_t fixedCost = 0u;
	for (uint32_t s = lane; s < CRX_LIT; s += 64u) fixedCost += sLit[s] * zipFixedLitBits(s);
	if (lane < CRX_DIST) fixedCost += 5u * sDist[lane];
	uint32_t dynamicCost = zipCodeLengths(sLit, CRX_LIT, 15u, sBits, lane);
	zipAssignCodes<15u>(sLit, CRX_LIT, sBits + 4u * CRX_LIT, lane);
	dynamicCost += zipCodeLengths(sDist, CRX_DIST, 15u, sBits, lane);
	zipAssignCodes<15u>(sDist, CRX_DIST, sBits + 4u * CRX_DIST, lane);
	uint32_t hlit = 0u, hdist = lane < CRX_DIST && sDist[lane] ? lane + 1u : 1u;          /* a segment without a match: HDIST = 1, one length of zero */
	for (uint32_t s = lane; s < CRX_LIT; s += 64u) if (sLit[s]) hlit = s + 1u;
	hlit = zipWaveMax(hlit); hdist = zipWaveMax(hdist);          /* (hlit >= 257: the end of block is used) */
	const uint32_t total = hlit + hdist;          /* <= 316 */
	uint32_t *const Q = sBits, *const R = sBits + 320u, *const clScratch = sBits + 640u;          /* the sequence; at a run's first position its length */
	for (uint32_t i = lane; i < total; i += 64u) Q[i] = (i < hlit ? sLit[i] : sDist[i - hlit]) & 15u;
	if (lane < 32u) sCl[lane] = 0u;
	__syncthreads();
	uint32_t start[5], carry = 0u;          /* where the run a position lies in starts */
#pragma unroll
	for (uint32_t t = 0u; t < 5u; ++t) {
		const uint32_t i = 64u * t + lane;
		const bool valid = i < total;
		const uint32_t v = valid ? Q[i] : 0u;
		uint32_t st = valid && (i == 0u || Q[i - 1u] != v) ? i : 0u;
		for (uint32_t d = 1u; d < 64u; d <<= 1) {
			const uint32_t o = __shfl_up(st, d);
			if (lane >= d && o > st) st = o;
		}
		if (carry > st) st = carry;
		carry = __shfl(st, 63);
		start[t] = st;
		if (valid && (i + 1u == total || Q[i + 1u] != v)) R[st] = i + 1u - st;
	}
	__syncthreads();
	uint32_t token[5], extraBits = 0u;          /* symbol | extra bits << 8 | their value << 16; 0xff: the position sends nothing */
#pragma unroll
	for (uint32_t t = 0u; t < 5u; ++t) {
		const uint32_t i = 64u * t + lane;
		uint32_t sym = 0xffu, eb = 0u, ex = 0u;
		if (i < total) {
			const uint32_t v = Q[i], o = i - start[t], r = R[start[t]];
			if (v == 0u) {
				const uint32_t in = o % 138u, block = zipMin(138u, r - (o - in));
				if (block >= 11u) { if (in == 0u) { sym = 18u; eb = 7u; ex = block - 11u; } }
				else if (block >= 3u) { if (in == 0u) { sym = 17u; eb = 3u; ex = block - 3u; } }
				else sym = 0u;
			} else if (o == 0u) sym = v;
			else {
				const uint32_t in = (o - 1u) % 6u, block = zipMin(6u, r - 1u - (o - 1u - in));
				if (block >= 3u) { if (in == 0u) { sym = 16u; eb = 2u; ex = block - 3u; } }
				else sym = v;
			}
		}
		token[t] = sym | eb << 8 | ex << 16;
		if (sym != 0xffu) { atomicAdd(&sCl[sym], 1u); extraBits += eb; }
	}
	__syncthreads();
	dynamicCost += extraBits + zipCodeLengths(sCl, CRX_CL, 7u, clScratch, lane);
	uint32_t *const clCount = clScratch + 4u * CRX_CL;
	const uint64_t used = (uint64_t)__ballot(lane < CRX_CL && sCl[lane] != 0u);
	if (__popcll((unsigned long long)used) == 1 && lane == 0u) { sCl[used & 1u ? 1u : 0u] = 1u; clCount[1] = 2u; }          /* the code-length code must be complete: a second symbol */
	__syncthreads();
	zipAssignCodes<7u>(sCl, CRX_CL, clCount, lane);
	const uint64_t sent = (uint64_t)__ballot(lane < CRX_CL && sCl[zipClOrder(lane < CRX_CL ? lane : 0u)] != 0u);
	uint32_t hclen = sent ? 64u - (uint32_t)__builtin_clzll((unsigned long long)sent) : 4u;
	if (hclen < 4u) hclen = 4u;
	dynamicCost = zipWaveSum(dynamicCost) + 14u + 3u * hclen;
	fixedCost = zipWaveSum(fixedCost);
	const bool dynamic = dynamicCost < fixedCost;
	const uint32_t sendLength = lane < hclen ? sCl[zipClOrder(lane)] & 15u : 0u;
	uint64_t code[5];
	uint32_t bits[5];
#pragma unroll
	for (uint32_t t = 0u; t < 5u; ++t) {
		const uint32_t sym = token[t] & 255u;
		code[t] = 0u; bits[t] = 0u;
		if (sym != 0xffu) {
			const uint32_t c = sCl[sym];
			bits[t] = (c & 15u) + ((token[t] >> 8) & 255u);
			code[t] = (uint64_t)(c >> 4) | (uint64_t)(token[t] >> 16) << (c & 15u);
		}
	}
	__syncthreads();          /* every read of the scratch and of the code-length code lies behind */
	for (uint32_t i = lane; i < CRX_SEG_OUT / 4u; i += 64u) sBits[i] = 0u;
	for (uint32_t i = lane; i < (1u << CRX_HASH_BITS); i += 64u) sHash[i] = 0u;
	if (!dynamic) {
		for (uint32_t s = lane; s < CRX_MAX_SYMBOLS; s += 64u) {
			uint64_t c = 0u;
			uint32_t small = 0u, b = 0u;
			if (s < 256u) zipLiteral(s, c, b);
			else { zipFixedLength(s, small, b); c = small; }
			sLit[s] = (uint32_t)c << 4 | b;
		}
		if (lane < 32u) sDist[lane] = zipRev(lane, 5u) << 4 | 5u;
	}
	__syncthreads();
	if (!dynamic) {
		if (lane == 0u) sBits[0] = (last ? 1u : 0u) | 2u;          /* BFINAL, BTYPE 01 */
		__syncthreads();
		return 3u;
	}
	if (lane == 0u) sBits[0] = (last ? 1u : 0u) | 4u | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13;          /* BFINAL, BTYPE 10, HLIT, HDIST, HCLEN */
	__syncthreads();
	uint32_t at = zipPut<false>(sBits, 17u, lane, sendLength, lane < hclen ? 3u : 0u);
#pragma unroll
	for (uint32_t t = 0u; t < 5u; ++t) at = zipPut<false>(sBits, at, lane, code[t], bits[t]);
	__syncthreads();
	return at;
}

/* One wave per segment. segOut: CRX_SEG_OUT bytes a segment; segMeta: {bytes, sum of the bytes mod 65521, sum of (len - p) * byte[p] mod 65521, 0} a segment.
 * DYNAMIC (crx_set_codes): the parse runs twice — ZIP_COUNT fills the histograms, zipChooseCodes makes the codes and decides, ZIP_TABLE emits —; nothing per
 * position is kept between the two. sLit, sDist, sCl: LDS of the dynamic kernel alone. */
template <bool DYNAMIC>
__device__ __forceinline__ void zipDeflate(const ZipGeom &G, const uint32_t *T, uint32_t *segOut, uint32_t *segMeta, uint32_t *sData, uint32_t *sHash, uint32_t *sBits,
                                           uint32_t *sLit, uint32_t *sDist, uint32_t *sCl) {
	const uint32_t k = blockIdx.x / G.segsPerChunk, seg = blockIdx.x - k * G.segsPerChunk;
	const uint32_t n = zipChunkBytes(G, k), begin = seg * CRX_SEG;
	if (begin >= n) return;          /* (the whole wave: a short last chunk has fewer segments) */
	const uint32_t len = zipMin(CRX_SEG, n - begin), lane = threadIdx.x;
	const bool last = begin + len == n;
	const uint32_t *const src = T + (size_t)k * G.pitch + begin / 4u;
	for (uint32_t i = lane; i < CRX_SEG / 4u + 4u; i += 64u) sData[i] = 4u * i < len ? src[i] : 0u;
	for (uint32_t i = lane; i < (1u << CRX_HASH_BITS); i += 64u) sHash[i] = 0u;
	if (DYNAMIC) {
		for (uint32_t i = lane; i < CRX_MAX_SYMBOLS; i += 64u) sLit[i] = i == 256u ? 1u : 0u;          /* the end of block */
		if (lane < 32u) sDist[lane] = 0u;
	} else for (uint32_t i = lane; i < CRX_SEG_OUT / 4u; i += 64u) sBits[i] = lane == 0u && i == 0u ? (last ? 1u : 0u) | 2u : 0u;          /* BFINAL, BTYPE 01 */
	__syncthreads();

	uint32_t sumA = 0u, sumB = 0u;          /* (sumB over the segment <= 255 * 4096 * 4097 / 2 < 2^31) */
	uint32_t at = 3u;                       /* bits written so far, wave-uniform */
	if (DYNAMIC) {
		zipParse<ZIP_COUNT>(sData, sHash, sBits, sLit, sDist, len, lane, 0u, sumA, sumB);
		__syncthreads();
		at = zipChooseCodes(sLit, sDist, sCl, sBits, sHash, last, lane);
		at = zipParse<ZIP_TABLE>(sData, sHash, sBits, sLit, sDist, len, lane, at, sumA, sumB);
		at = zipPut<false>(sBits, at, lane, sLit[256] >> 4, lane == 0u ? sLit[256] & 15u : 0u);          /* end of block */
	} else {
		at = zipParse<ZIP_FIXED>(sData, sHash, sBits, nullptr, nullptr, len, lane, at, sumA, sumB);
		at += 7u;          /* end of block: seven zero bits */
	}
	if (!last) {
		at = (at + 3u + 7u) & ~7u;          /* an empty stored block: BFINAL 0, BTYPE 00, to the byte boundary, LEN 0000, NLEN ffff */
		if (lane == 0u) {
			const uint64_t v = (uint64_t)0xffffu << ((at + 16u) & 31u);
			atomicOr(&sBits[(at + 16u) >> 5], (uint32_t)v);
			if (v >> 32) atomicOr(&sBits[((at + 16u) >> 5) + 1u], (uint32_t)(v >> 32));
		}
		at += 32u;
	} else at = (at + 7u) & ~7u;
	__syncthreads();
	const uint32_t bytes = at >> 3;
	uint32_t *const dst = segOut + (size_t)blockIdx.x * (CRX_SEG_OUT / 4u);
	for (uint32_t i = lane; i < (bytes + 3u) / 4u; i += 64u) dst[i] = sBits[i];
	sumA = zipWaveSum(sumA); sumB = zipWaveSum(sumB);
	if (lane == 0u) {
		uint32_t *const meta = segMeta + 4u * (size_t)blockIdx.x;
		meta[0] = bytes; meta[1] = sumA % CRX_ADLER; meta[2] = sumB % CRX_ADLER; meta[3] = 0u;
	}
}

__global__ __launch_bounds__(64) void k_zip_deflate(const ZipGeom G, const uint32_t *T, uint32_t *segOut, uint32_t *segMeta) {
	__shared__ uint32_t sData[CRX_SEG / 4u + 4u];
	__shared__ uint32_t sHash[1u << CRX_HASH_BITS];         /* position + 1 of the last occurrence in an earlier step, 0: none */
	__shared__ uint32_t sBits[CRX_SEG_OUT / 4u];
	zipDeflate<false>(G, T, segOut, segMeta, sData, sHash, sBits, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void k_zip_deflate_dynamic(const ZipGeom G, const uint32_t *T, uint32_t *segOut, uint32_t *segMeta) {
	__shared__ uint32_t sData[CRX_SEG / 4u + 4u];
	__shared__ uint32_t sHash[1u << CRX_HASH_BITS];
	__shared__ uint32_t sBits[CRX_SEG_OUT / 4u];
	__shared__ uint32_t sLit[CRX_MAX_SYMBOLS], sDist[32], sCl[32];          /* histograms, then code tables */
	zipDeflate<true>(G, T, segOut, segMeta, sData, sHash, sBits, sLit, sDist, sCl);
}

/* crx_debug_code_lengths: one wave a histogram through zipCodeLengths, the function zipChooseCodes calls */
__global__ __launch_bounds__(64) void k_zip_code_lengths(const uint32_t *freq, uint32_t symbols, uint32_t limit, uint8_t *lengths) {
	__shared__ uint32_t sTab[CRX_MAX_SYMBOLS];
	__shared__ uint32_t sScratch[CRX_LEN_SCRATCH(CRX_MAX_SYMBOLS)];
	for (uint32_t s = threadIdx.x; s < symbols; s += 64u) sTab[s] = freq[(size_t)blockIdx.x * symbols + s];
	__syncthreads();
	zipCodeLengths(sTab, symbols, limit, sScratch, threadIdx.x);
	for (uint32_t s = threadIdx.x; s < symbols; s += 64u) lengths[(size_t)blockIdx.x * symbols + s] = (uint8_t)sTab[s];
}

/* One workgroup. segOff: where a segment's bytes start in its chunk's deflate data; chunkInfo: {size, raw, Adler-32, 0} a chunk;
 * chunkPos: [nchunks] positions in the output, [nchunks] byte counts (8 + size), [1] the total */
__global__ __launch_bounds__(256) void k_zip_scan(const ZipGeom G, const uint32_t *segMeta, uint32_t *segOff, uint32_t *chunkInfo, uint64_t *chunkPos) {
	for (uint32_t k = threadIdx.x; k < G.nchunks; k += 256u) {
		const uint32_t n = zipChunkBytes(G, k), segs = (n + CRX_SEG - 1u) / CRX_SEG;
		uint32_t a = 1u, b = 0u, off = 0u;          /* (off <= segs * CRX_SEG_OUT < 2^32 for n < 2^31) */
		for (uint32_t s = 0; s < segs && !G.allRaw; ++s) {
			const size_t at = (size_t)k * G.segsPerChunk + s;
			const uint32_t *const meta = segMeta + 4u * at;
			segOff[at] = off;
			off += meta[0];
			b = (b + zipMin(CRX_SEG, n - s * CRX_SEG) * a + meta[2]) % CRX_ADLER;          /* Adler-32 of a concatenation */
			a = (a + meta[1]) % CRX_ADLER;
		}
		const uint64_t stream = 2u + (uint64_t)off + 4u;
		const bool raw = G.allRaw || stream >= n;
		uint32_t *const info = chunkInfo + 4u * (size_t)k;
		info[0] = raw ? n : (uint32_t)stream; info[1] = raw ? 1u : 0u; info[2] = b << 16 | a; info[3] = 0u;
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		uint64_t pos = 0u;
		for (uint32_t k = 0; k < G.nchunks; ++k) {
			const uint64_t bytes = 8u + (uint64_t)chunkInfo[4u * (size_t)k];
			chunkPos[k] = pos; chunkPos[G.nchunks + k] = bytes;
			pos += bytes;
		}
		chunkPos[2u * (size_t)G.nchunks] = pos;
	}
}

__device__ __forceinline__ void zipStore4(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* One workgroup per segment: its bytes to their place in the output. MIXED: rows with HALF channels (off: their prefix table in LDS) */
template <bool MIXED>
__device__ __forceinline__ void zipEmit(const ZipArgs &A, const ZipGeom &G, const uint32_t *off, const uint32_t *segOut, const uint32_t *segMeta, const uint32_t *segOff,
                                        const uint32_t *chunkInfo, const uint64_t *chunkPos, uint8_t *out) {
	const uint32_t k = blockIdx.x / G.segsPerChunk, seg = blockIdx.x - k * G.segsPerChunk;
	const uint32_t n = zipChunkBytes(G, k), begin = seg * CRX_SEG;
	if (begin >= n) return;
	const uint32_t size = chunkInfo[4u * (size_t)k], raw = chunkInfo[4u * (size_t)k + 1u], adler = chunkInfo[4u * (size_t)k + 2u];
	uint8_t *const chunk = out + chunkPos[k];
	if (seg == 0u && threadIdx.x == 0u) {
		zipStore4(chunk, G.firstRow + k * G.lpc);
		zipStore4(chunk + 4, size);
		if (!raw) {
			chunk[8] = 0x78; chunk[9] = 0x01;
			uint8_t *const t = chunk + 8u + size - 4u;
			t[0] = (uint8_t)(adler >> 24); t[1] = (uint8_t)(adler >> 16); t[2] = (uint8_t)(adler >> 8); t[3] = (uint8_t)adler;
		}
	}
	if (raw && MIXED) {
		const uint32_t bytes = zipMin(CRX_SEG, n - begin);          /* even */
		ZipHeld h = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
		for (uint32_t w = threadIdx.x; 4u * w < bytes; w += 256u) {
			uint8_t *const to = chunk + 8u + begin + 4u * w;
			for (uint32_t b = 0; b < 4u && 4u * w + b < bytes; ++b) to[b] = (uint8_t)zipMixedByte(A, G, off, k, begin + 4u * w + b, h);          /* a last 2-byte store */
		}
	} else if (raw) {
		const uint32_t words = zipMin(CRX_SEG, n - begin) / 4u;
		for (uint32_t w = threadIdx.x; w < words; w += 256u) zipStore4(chunk + 8u + begin + 4u * w, zipRawWord(A, G, k, begin / 4u + w));
	} else {
		const uint32_t bytes = segMeta[4u * (size_t)blockIdx.x];
		const uint8_t *const from = (const uint8_t *)(segOut + (size_t)blockIdx.x * (CRX_SEG_OUT / 4u));
		uint8_t *const to = chunk + 10u + segOff[blockIdx.x];
		for (uint32_t i = threadIdx.x; i < bytes; i += 256u) to[i] = from[i];
	}
}

__global__ __launch_bounds__(256) void k_zip_emit(const ZipArgs A, const ZipGeom G, const uint32_t *segOut, const uint32_t *segMeta, const uint32_t *segOff,
                                                  const uint32_t *chunkInfo, const uint64_t *chunkPos, uint8_t *out) {
	zipEmit<false>(A, G, nullptr, segOut, segMeta, segOff, chunkInfo, chunkPos, out);
}

__global__ __launch_bounds__(256) void k_zip_emit_mixed(const ZipArgs A, const ZipRow R, const ZipGeom G, const uint32_t *segOut, const uint32_t *segMeta, const uint32_t *segOff,
                                                        const uint32_t *chunkInfo, const uint64_t *chunkPos, uint8_t *out) {
	__shared__ uint32_t sOff[CRH_PACK_MAX_CHANNELS + 1u];
	if (threadIdx.x <= G.nch) sOff[threadIdx.x] = R.off[threadIdx.x];
	__syncthreads();
	zipEmit<true>(A, G, sOff, segOut, segMeta, segOff, chunkInfo, chunkPos, out);
}
#endif          /* CRX_ZIP_CONVERSION_ONLY */
